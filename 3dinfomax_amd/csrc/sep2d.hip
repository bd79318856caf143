// Multi-conformer losses with one 2D embedding per conformer: NTXentMultiplePositivesSeparate2D (reference commons/losses.py:692-744)
// and NTXentMMDSeparate2D (reference commons/losses.py:394-476).  B molecules, C conformers, N = B C points per view, D features.
//
//   row normalise   y = x / max(|x|, 1e-12) (F.normalize), one wave per row; backward dx = (dy - y (y . dy)) / |x|, or dy / 1e-12
//                   below the clamp.
//   Separate2D      S [N, N] = z1v z2^T comes from the GEMM; rows (i, l), columns (j, u).  forward: one workgroup per molecule i sums
//                   P = exp(S / (|z1||z2|) / tau) over its C rows: den_i over the columns of the other molecules (the whole C x C
//                   diagonal block is left out), pos_i over the matched conformers (j, u) = (i, l); then one workgroup sums
//                   -log(pos_i / den_i) in order.  backward: one workgroup per row writes dS and the row's norm coefficient, then the
//                   column coefficients from dS in a pass of their own.
//   MMD             X = the 2D view [N, D], Y = the 3D view [N, D].  Entry [a, b] of the similarity matrix compares the C points
//                   X[b] with the C points Y[a] (rows index the 3D view).  forward: cross[(a, u), (b, l)] = |Y[a, u] - X[b, l]|^2 by
//                   direct differences (a Gram form cancels when conformers nearly coincide), tiled through LDS; intra[v, m, l, l'] the
//                   same inside one molecule of one view; then one thread per (a, b): bandwidth from the sum of the (2C)^2 squared
//                   distances, the kernel sums, mmd, sim = 1 / (mmd + 1).  backward (the bandwidth is a constant): one thread per
//                   (a, b) writes gcross = dL/d cross; one workgroup per molecule and view sums dL/d intra over the partner molecules
//                   in order; dY[r] = 2 sum_c gcross[r, c] (Y[r] - X[c]) + the intra terms, and dX from the transposed gcross,
//                   again by direct differences and in a fixed order.
// Nothing scales with B^2 C^2 D: the largest buffers are cross and gcross, B^2 C^2 floats each.  No atomics anywhere.
#include "common.h"

#include <math.h>

namespace i3d {

constexpr int S2_MAX_CONF = 8;
constexpr double S2_NORM_EPS = 1e-12;

// ---- row normalise ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
row_normalize_fwd_kernel(const float* __restrict__ x, int rows, int dim, float* __restrict__ y, float* __restrict__ norms) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * dim;
    double acc = 0.;
    for (int c = lane; c < dim; c += 64) acc += (double)xr[c] * (double)xr[c];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    const float n = (float)sqrt(acc);
    const float den = n > (float)S2_NORM_EPS ? n : (float)S2_NORM_EPS;
    for (int c = lane; c < dim; c += 64) y[r * dim + c] = xr[c] / den;
    if (lane == 0) norms[r] = n;
}

__global__ void __launch_bounds__(256)
row_normalize_bwd_kernel(const float* __restrict__ x, const float* __restrict__ norms, const float* __restrict__ grad_y, int rows,
                         int dim, float* __restrict__ grad_x) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * dim;
    const float* gr = grad_y + r * dim;
    const float n = norms[r];
    if (!(n > (float)S2_NORM_EPS)) {          // the clamp is active: y = x / 1e-12, the norm carries no gradient
        for (int c = lane; c < dim; c += 64) grad_x[r * dim + c] = gr[c] / (float)S2_NORM_EPS;
        return;
    }
    double dot = 0.;
    for (int c = lane; c < dim; c += 64) dot += (double)xr[c] * (double)gr[c];
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
    const double inv = 1. / (double)n, k = dot * inv * inv;          // (y . dy) / |x| = (x . dy) / |x|^2 ... times y = x / |x| below
    for (int c = lane; c < dim; c += 64) grad_x[r * dim + c] = (float)(((double)gr[c] - k * (double)xr[c]) * inv);
}

// ---- Separate2D ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sep2d_fwd_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2, int B, int C,
                 double inv_tau, double* __restrict__ row_den, double* __restrict__ row_pos) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int i = blockIdx.x;
    const long N = (long)B * C;
    const long c_lo = (long)i * C, c_hi = c_lo + C;
    double den = 0., pos = 0.;
    for (int l = 0; l < C; ++l) {
        const long r = c_lo + l;
        const double a = (double)n1[r];
        for (long c = threadIdx.x; c < N; c += 256) {
            const bool own = c >= c_lo && c < c_hi;
            if (own && c != r) continue;          // the rest of the diagonal block is in neither sum
            const double p = exp((double)sim[r * N + c] / (a * (double)n2[c]) * inv_tau);
            if (own) pos += p;
            else den += p;
        }
    }
    den = block_sum_f64(den, sm);
    pos = block_sum_f64(pos, sm);
    if (threadIdx.x == 0) {
        row_den[i] = den;
        row_pos[i] = pos;
    }
}

__global__ void __launch_bounds__(256)
sep2d_loss_kernel(const double* __restrict__ row_den, const double* __restrict__ row_pos, int B, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.;
    for (int i = threadIdx.x; i < B; i += 256) acc -= log(row_pos[i] / row_den[i]);
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(acc / (double)B);
}

// dL/dP[(i, l), (j, u)] = g / (B den_i) for j != i, -g / (B pos_i) for the matched conformer, 0 in the rest of the diagonal block;
// G = dL/dP P / tau, dS = H = G / (a b), ca_r = -(1 / a) sum_c H s' b (s' = S / (a b)): the norm path of row r
__global__ void __launch_bounds__(256)
sep2d_bwd_row_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
                     const double* __restrict__ row_den, const double* __restrict__ row_pos, int B, int C, double inv_tau,
                     const float* __restrict__ gs_dev, float* __restrict__ dsim, float* __restrict__ ca) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long r = blockIdx.x;
    const long N = (long)B * C;
    const int i = (int)(r / C);
    const long c_lo = (long)i * C, c_hi = c_lo + C;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / (double)B;
    const double g_neg = gs / row_den[i], g_pos = -gs / row_pos[i];
    const double a = (double)n1[r];
    double da = 0.;
    for (long c = threadIdx.x; c < N; c += 256) {
        const bool own = c >= c_lo && c < c_hi;
        float h = 0.f;
        if (!own || c == r) {
            const double b = (double)n2[c], nrm = a * b;
            const double s = (double)sim[r * N + c] / nrm;
            const double H = (own ? g_pos : g_neg) * exp(s * inv_tau) * inv_tau / nrm;
            h = (float)H;
            da -= H * s * b;
        }
        dsim[r * N + c] = h;
    }
    da = block_sum_f64(da, sm);
    if (threadIdx.x == 0) ca[r] = a > 0. ? (float)(da / a) : 0.f;
}

// cb_c = -(1 / b_c) sum_r H[r, c] s'[r, c] a_r: 16 columns per workgroup, 16 row lanes, the lanes' partials summed in order
constexpr int S2_COL_W = 16, S2_COL_L = 16;
__global__ void __launch_bounds__(256)
sep2d_bwd_col_kernel(const float* __restrict__ sim, const float* __restrict__ dsim, const float* __restrict__ n1,
                     const float* __restrict__ n2, long N, float* __restrict__ cb) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[S2_COL_L][S2_COL_W];
    const int cx = threadIdx.x % S2_COL_W, ry = threadIdx.x / S2_COL_W;
    const long c = (long)blockIdx.x * S2_COL_W + cx;
    double acc = 0.;
    if (c < N) {
        const double b = (double)n2[c];
        for (long r = ry; r < N; r += S2_COL_L) {
            const double a = (double)n1[r];
            acc -= (double)dsim[r * N + c] * ((double)sim[r * N + c] / (a * b)) * a;
        }
    }
    sm[ry][cx] = acc;
    __syncthreads();
    if (ry == 0 && c < N) {
        const double b = (double)n2[c];
        double t = 0.;
        for (int k = 0; k < S2_COL_L; ++k) t += sm[k][cx];
        cb[c] = b > 0. ? (float)(t / b) : 0.f;
    }
}

// ---- MMD ----------------------------------------------------------------------------------------------------------------------
// cross[r, c] = sum_d (Y[r, d] - X[c, d])^2: a 64 x 64 tile per workgroup, 4 x 4 outputs per thread (rows ty + 16 i, columns tx + 16 j:
// LDS rows of 33 words, no bank conflicts), the feature axis in chunks of 32 through LDS
constexpr int CR_T = 64, CR_K = 32;
__global__ void __launch_bounds__(256)
mmd_cross_l2_kernel(const float* __restrict__ Y, const float* __restrict__ X, int N, int D, float* __restrict__ cross) {
    I3D_CHAIN_PRIO();
    __shared__ float ys[CR_T][CR_K + 1], xs[CR_T][CR_K + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long r0 = (long)blockIdx.y * CR_T, c0 = (long)blockIdx.x * CR_T;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += CR_K) {
        __syncthreads();
        for (int e = threadIdx.x; e < CR_T * CR_K; e += 256) {
            const int rr = e / CR_K, dd = e - rr * CR_K;
            const bool dok = d0 + dd < D;
            ys[rr][dd] = (dok && r0 + rr < N) ? Y[(r0 + rr) * D + d0 + dd] : 0.f;
            xs[rr][dd] = (dok && c0 + rr < N) ? X[(c0 + rr) * D + d0 + dd] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int dd = 0; dd < CR_K; ++dd) {
            float yv[4], xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                yv[i] = ys[ty + 16 * i][dd];
                xv[i] = xs[tx + 16 * i][dd];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float df = yv[i] - xv[j];
                    acc[i][j] = fmaf(df, df, acc[i][j]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long r = r0 + ty + 16 * i, c = c0 + tx + 16 * j;
            if (r < N && c < N) cross[r * N + c] = acc[i][j];
        }
}

// intra[v, m, l, l'] = |P_v[m, l] - P_v[m, l']|^2 (v = 0: X, v = 1: Y), one thread per entry
__global__ void __launch_bounds__(256)
mmd_intra_l2_kernel(const float* __restrict__ X, const float* __restrict__ Y, int B, int C, int D, float* __restrict__ intra) {
    I3D_CHAIN_PRIO();
    const long per = (long)B * C * C;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * per) return;
    const int v = t >= per;
    const long e = t - v * per;
    const long m = e / (C * C);
    const int q = (int)(e - m * C * C), l = q / C, l2 = q - l * C;
    const float* P = v ? Y : X;
    const float* p = P + (m * C + l) * D;
    const float* p2 = P + (m * C + l2) * D;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) {
        const float df = p[d] - p2[d];
        acc = fmaf(df, df, acc);
    }
    intra[t] = acc;
}

// sum_k exp(-L / (bw mul^k))
__device__ __forceinline__ double mmd_kernel_sum(double L, double bw, double mul, int num) {
    double s = 0.;
    for (int k = 0; k < num; ++k) {
        s += exp(-L / bw);
        bw *= mul;
    }
    return s;
}

// d/dL of the above
__device__ __forceinline__ double mmd_kernel_dsum(double L, double bw, double mul, int num) {
    double s = 0.;
    for (int k = 0; k < num; ++k) {
        s -= exp(-L / bw) / bw;
        bw *= mul;
    }
    return s;
}

// one thread per (a, b): the 2C points are X[b] then Y[a]
__global__ void __launch_bounds__(256)
mmd_pair_fwd_kernel(const float* __restrict__ cross, const float* __restrict__ intra, int B, int C, int num, double mul,
                    double bw_div, float* __restrict__ bandwidth, float* __restrict__ sim) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * B) return;
    const long a = t / B, b = t - a * B;
    const int CC = C * C;
    const long N = (long)B * C;
    const float* LX = intra + b * CC;
    const float* LY = intra + ((long)B + a) * CC;
    const float* LC = cross + a * C * N + b * C;
    double tot = 0., cr = 0.;
    for (int q = 0; q < CC; ++q) tot += (double)LX[q] + (double)LY[q];
    for (int u = 0; u < C; ++u)
        for (int l = 0; l < C; ++l) cr += (double)LC[u * N + l];
    const float bwf = (float)((tot + 2. * cr) / (double)(4 * CC - 2 * C) / bw_div);
    const double bw = (double)bwf;
    double same = 0., diff = 0.;
    for (int q = 0; q < CC; ++q) same += mmd_kernel_sum((double)LX[q], bw, mul, num) + mmd_kernel_sum((double)LY[q], bw, mul, num);
    for (int u = 0; u < C; ++u)
        for (int l = 0; l < C; ++l) diff += mmd_kernel_sum((double)LC[u * N + l], bw, mul, num);
    const double mmd = (same - 2. * diff) / (double)CC;
    bandwidth[t] = bwf;
    sim[t] = (float)(1. / (mmd + 1.));
}

// gcross[(a, u), (b, l)] = dL/d cross = dmmd[a, b] (-2 / C^2) K'(cross), dmmd = -dsim sim^2
__global__ void __launch_bounds__(256)
mmd_pair_bwd_kernel(const float* __restrict__ cross, const float* __restrict__ bandwidth, const float* __restrict__ sim,
                    const float* __restrict__ dsim, int B, int C, int num, double mul, float* __restrict__ gcross) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * B) return;
    const long a = t / B, b = t - a * B;
    const long N = (long)B * C;
    const long off = a * C * N + b * C;
    const double s = (double)sim[t], bw = (double)bandwidth[t];
    const double coef = -(double)dsim[t] * s * s * (-2. / (double)(C * C));
    for (int u = 0; u < C; ++u)
        for (int l = 0; l < C; ++l)
            gcross[off + u * N + l] = (float)(coef * mmd_kernel_dsum((double)cross[off + u * N + l], bw, mul, num));
}

// gintra[v, m, l, l'] = (2 / C^2) sum_j dmmd[pair of m and j] K'(intra[v, m, l, l'], bandwidth of that pair): both ordered entries of the
// symmetric block.  v = 0 (X, m is the column b of the similarity matrix): j runs over the rows a; v = 1 (Y, m is the row a): over the
// columns b.  One workgroup per (m, v); the partner molecules strided over the threads, summed in a fixed order.
__global__ void __launch_bounds__(256)
mmd_intra_bwd_kernel(const float* __restrict__ intra, const float* __restrict__ bandwidth, const float* __restrict__ sim,
                     const float* __restrict__ dsim, int B, int C, int num, double mul, float* __restrict__ gintra) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int m = blockIdx.x, v = blockIdx.y;
    const int CC = C * C;
    const long base = ((long)v * B + m) * CC;
    if ((int)threadIdx.x < C) gintra[base + threadIdx.x * C + threadIdx.x] = 0.f;
    for (int l = 0; l < C; ++l)
        for (int l2 = l + 1; l2 < C; ++l2) {
            const double L = (double)intra[base + l * C + l2];
            double acc = 0.;
            for (int j = threadIdx.x; j < B; j += 256) {
                const long idx = v ? (long)m * B + j : (long)j * B + m;
                const double s = (double)sim[idx];
                acc += -(double)dsim[idx] * s * s * mmd_kernel_dsum(L, (double)bandwidth[idx], mul, num);
            }
            acc = block_sum_f64(acc, sm);
            if (threadIdx.x == 0) {
                const float g = (float)(acc * 2. / (double)CC);
                gintra[base + l * C + l2] = g;
                gintra[base + l2 * C + l] = g;
            }
        }
}

// out[r, d] = 2 (sum_c G(r, c) (own[r, d] - other[c, d]) + sum_l' GI[m, l, l'] (own[r, d] - own[m C + l', d])), r = m C + l;
// G(r, c) = gcross[r, c] (TRANS = false: own = Y) or gcross[c, r] (TRANS = true: own = X).  GR rows per workgroup, one feature
// per thread (blockIdx.y: chunks of 256 features), the columns in ascending order through an LDS tile of G.
constexpr int GR = 8, GCOLS = 64;
template <bool TRANS>
__global__ void __launch_bounds__(256)
mmd_grad_kernel(const float* __restrict__ gcross, const float* __restrict__ GI, const float* __restrict__ own,
                const float* __restrict__ other, int N, int C, int D, float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ float g[GR][GCOLS];
    const long r0 = (long)blockIdx.x * GR;
    const int d = blockIdx.y * 256 + threadIdx.x;
    const bool dok = d < D;
    float y[GR];
    double acc[GR];
#pragma unroll
    for (int rr = 0; rr < GR; ++rr) {
        y[rr] = (dok && r0 + rr < N) ? own[(r0 + rr) * D + d] : 0.f;
        acc[rr] = 0.;
    }
    for (long c0 = 0; c0 < N; c0 += GCOLS) {
        __syncthreads();
        for (int e = threadIdx.x; e < GR * GCOLS; e += 256) {
            const int rr = TRANS ? e % GR : e / GCOLS, cc = TRANS ? e / GR : e % GCOLS;
            const long r = r0 + rr, c = c0 + cc;
            g[rr][cc] = (r < N && c < N) ? (TRANS ? gcross[c * N + r] : gcross[r * N + c]) : 0.f;
        }
        __syncthreads();
        if (!dok) continue;
        const int ncol = (int)((N - c0) < GCOLS ? (N - c0) : GCOLS);
        for (int cc = 0; cc < ncol; ++cc) {
            const float x = other[(c0 + cc) * D + d];
#pragma unroll
            for (int rr = 0; rr < GR; ++rr) acc[rr] += (double)g[rr][cc] * (double)(y[rr] - x);
        }
    }
    if (!dok) return;
#pragma unroll
    for (int rr = 0; rr < GR; ++rr) {
        const long r = r0 + rr;
        if (r >= N) continue;
        const long m = r / C;
        const int l = (int)(r - m * C);
        double s = acc[rr];
        for (int l2 = 0; l2 < C; ++l2)
            s += (double)GI[(m * C + l) * C + l2] * (double)(y[rr] - own[(m * C + l2) * D + d]);
        out[r * D + d] = (float)(2. * s);
    }
}

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_row_normalize_fwd(const float* x, int rows, int dim, float* y, float* norms, void* stream) {
    I3D_CHECK_ARG(rows >= 0 && dim > 0, "bad shape");
    if (rows == 0) return I3D_OK;
    I3D_CHECK_ARG(x && y && norms, "null pointer");
    hipLaunchKernelGGL(row_normalize_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, dim, y, norms);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_row_normalize_bwd(const float* x, const float* norms, const float* grad_y, int rows, int dim, float* grad_x,
                                     void* stream) {
    I3D_CHECK_ARG(rows >= 0 && dim > 0, "bad shape");
    if (rows == 0) return I3D_OK;
    I3D_CHECK_ARG(x && norms && grad_y && grad_x, "null pointer");
    hipLaunchKernelGGL(row_normalize_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, norms, grad_y, rows, dim,
                       grad_x);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_sep2d_max_conformers(void) { return S2_MAX_CONF; }

static int sep2d_check(int batch, int conf) {
    I3D_CHECK_ARG(batch >= 2, "fewer than two molecules");
    I3D_CHECK_ARG(conf >= 1 && conf <= S2_MAX_CONF, "conformers per molecule outside 1..8");
    I3D_CHECK_ARG((long)batch * conf <= 46340, "batch * conformers above 46340: the [BC, BC] matrix would pass 2^31 entries");
    return I3D_OK;
}

extern "C" int i3d_sep2d_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, float tau, double* row_den,
                             double* row_pos, float* loss, void* stream) {
    if (int rc = sep2d_check(batch, conf)) return rc;
    I3D_CHECK_ARG(tau > 0.f, "tau must be positive");
    I3D_CHECK_ARG(sim && n1 && n2 && row_den && row_pos && loss, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sep2d_fwd_kernel, dim3(batch), dim3(256), 0, s, sim, n1, n2, batch, conf, 1. / (double)tau, row_den, row_pos);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(sep2d_loss_kernel, dim3(1), dim3(256), 0, s, row_den, row_pos, batch, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_sep2d_bwd(const float* sim, const float* n1, const float* n2, const double* row_den, const double* row_pos,
                             int batch, int conf, float tau, const float* grad_scale, float* dsim, float* ca, float* cb,
                             void* stream) {
    if (int rc = sep2d_check(batch, conf)) return rc;
    I3D_CHECK_ARG(tau > 0.f, "tau must be positive");
    I3D_CHECK_ARG(sim && n1 && n2 && row_den && row_pos && dsim && ca && cb, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long N = (long)batch * conf;
    hipLaunchKernelGGL(sep2d_bwd_row_kernel, dim3((unsigned)N), dim3(256), 0, s, sim, n1, n2, row_den, row_pos, batch, conf,
                       1. / (double)tau, grad_scale, dsim, ca);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(sep2d_bwd_col_kernel, dim3(cdiv(N, S2_COL_W)), dim3(256), 0, s, sim, dsim, n1, n2, N, cb);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

static int mmd_check(int batch, int conf, int dim, int kernel_num, double kernel_mul) {
    if (int rc = sep2d_check(batch, conf)) return rc;
    I3D_CHECK_ARG(dim >= 1, "feature count below 1");
    I3D_CHECK_ARG(kernel_num >= 1 && kernel_num <= 64, "kernel_num outside 1..64");
    I3D_CHECK_ARG(kernel_mul > 0., "kernel_mul must be positive");
    return I3D_OK;
}

extern "C" int i3d_mmd_pair_fwd(const float* X, const float* Y, int batch, int conf, int dim, int kernel_num, double kernel_mul,
                                float* cross, float* intra, float* bandwidth, float* sim, void* stream) {
    if (int rc = mmd_check(batch, conf, dim, kernel_num, kernel_mul)) return rc;
    I3D_CHECK_ARG(X && Y && cross && intra && bandwidth && sim, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = batch * conf;
    hipLaunchKernelGGL(mmd_cross_l2_kernel, dim3(cdiv(N, CR_T), cdiv(N, CR_T)), dim3(256), 0, s, Y, X, N, dim, cross);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(mmd_intra_l2_kernel, dim3(cdiv(2L * N * conf, 256)), dim3(256), 0, s, X, Y, batch, conf, dim, intra);
    I3D_CHECK_LAUNCH();
    const double bw_div = pow(kernel_mul, (double)(kernel_num / 2));
    hipLaunchKernelGGL(mmd_pair_fwd_kernel, dim3(cdiv((long)batch * batch, 256)), dim3(256), 0, s, cross, intra, batch, conf,
                       kernel_num, kernel_mul, bw_div, bandwidth, sim);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_mmd_pair_bwd(const float* X, const float* Y, const float* cross, const float* intra, const float* bandwidth,
                                const float* sim, const float* dsim, int batch, int conf, int dim, int kernel_num,
                                double kernel_mul, float* gcross, float* gintra, float* dX, float* dY, void* stream) {
    if (int rc = mmd_check(batch, conf, dim, kernel_num, kernel_mul)) return rc;
    I3D_CHECK_ARG(X && Y && cross && intra && bandwidth && sim && dsim && gcross && gintra && dX && dY, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = batch * conf;
    hipLaunchKernelGGL(mmd_pair_bwd_kernel, dim3(cdiv((long)batch * batch, 256)), dim3(256), 0, s, cross, bandwidth, sim, dsim,
                       batch, conf, kernel_num, kernel_mul, gcross);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(mmd_intra_bwd_kernel, dim3(batch, 2), dim3(256), 0, s, intra, bandwidth, sim, dsim, batch, conf, kernel_num,
                       kernel_mul, gintra);
    I3D_CHECK_LAUNCH();
    const dim3 grid(cdiv(N, GR), cdiv(dim, 256));
    const float* gix = gintra;
    const float* giy = gintra + (long)batch * conf * conf;
    hipLaunchKernelGGL(mmd_grad_kernel<false>, grid, dim3(256), 0, s, gcross, giy, Y, X, N, conf, dim, dY);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(mmd_grad_kernel<true>, grid, dim3(256), 0, s, gcross, gix, X, Y, N, conf, dim, dX);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
