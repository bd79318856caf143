// The non-contrastive objectives: statistics over the batch axis (column family) and one L2 normalisation per row (row family).
//
// Replaces the forward of BarlowTwinsLoss (reference commons/losses.py:45-73), CosineSimilarityLoss (:76-95), CriticLoss (:33-42) and the
// std_loss / cov_loss terms (:954-964) that RegularizationLoss (:98-123) turns on by default.
//
// Column family, z [n, dim], both views in one launch:
//     moments   mean_j, var_j = sum_i (z_ij - mean_j)^2 / (n - 1): the mean first, then the centred squares, both in fp64 (never
//               E[x^2] - E[x]^2); writes a = (z - mean) / std (BarlowTwins) and / or c = z - mean (covariance term)
//     pass      over M [dim, dim] = a^T b resp. c^T c from the library's GEMM: C = M inv_n,
//               partial += w_diag (C_ii - target)^2 + w_off sum_{i != j} C_ij^2;  M is overwritten with G = d partial / dC
//     finish    loss = scale sum(partials) + var_w / dim sum_{views, j} relu(1 - sqrt(var_j + 1e-4))
//     backward  two GEMMs da = b G^T, db = a G (covariance: dc = c G, G symmetric), then one launch for both views:
//               dz = g [sa (da - mean(da) - a sum(da a) / (n - 1)) / std + sc (dc - mean(dc)) + hc_j (z - mean_j)],
//               hc_j = -var_w / (dim (n - 1) sqrt(var_j + 1e-4)) on the active side of the hinge, g the upstream gradient read on the device
// A column workgroup is 16 columns x 16 row lanes: the 16 lanes of a row read 16 consecutive floats, a wave four such rows.
//
// Row family, x [rows, dim], y [rows, dim, reps] (reps == 1: the other view; CriticLoss: the reconstructions, normalised over dim, the
// elements of one vector reps floats apart):
//     l_b = sum_r sum_d (x_d / max(|x|, 1e-12) - y_dr / max(|y_r|, 1e-12))^2, one workgroup per row, y read in memory order
//     backward  one launch for dx and dy; a norm below the clamp has the constant denominator 1e-12 there too (F.normalize)
// Neither the [rows, dim, reps] repeat of x nor a transposed copy of y exists.
//
// Every sum is fp64 in a fixed order, no atomics: the same bits on every run.
#include "common.h"

namespace i3d {
namespace {

constexpr int BS_CW = 16, BS_RL = 16;          // column workgroups: 16 columns x 16 row lanes
constexpr int BS_PASS_CHUNK = 2048;            // elements of a dim x dim matrix per workgroup of the pass
constexpr int BS_MAX_REPS = 32;                // reconstructions per row
constexpr double BS_NORM_EPS = 1e-12;          // F.normalize
constexpr double BS_VAR_EPS = 1e-4;            // std_loss

struct BsViews {
    const float* z[2];
    float* a[2];
    float* c[2];
};

struct BsBwd {
    const float* z[2];
    const float* a[2];
    const float* da[2];
    const float* dc[2];
    float* dz[2];
};

// the column's total over the 16 row lanes, in lane order, to every thread of the column
__device__ __forceinline__ double col_sum(double v, double (*sm)[BS_CW], int ry, int cx) {
    __syncthreads();
    sm[ry][cx] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < BS_RL; ++k) t += sm[k][cx];
    return t;
}

// mom [views, 2, dim] (fp64): mean, unbiased variance
__global__ void __launch_bounds__(256)
bs_moments_kernel(BsViews v, int n, int dim, double* __restrict__ mom) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[BS_RL][BS_CW];
    const int view = blockIdx.y, cx = threadIdx.x % BS_CW, ry = threadIdx.x / BS_CW;
    const int j = blockIdx.x * BS_CW + cx;
    const bool ok = j < dim;
    const float* z = v.z[view] + (ok ? j : 0);
    double s = 0.0;
    if (ok)
        for (int i = ry; i < n; i += BS_RL) s += (double)z[(long)i * dim];
    const double mean = col_sum(s, sm, ry, cx) / n;
    double q = 0.0;
    if (ok)
        for (int i = ry; i < n; i += BS_RL) {
            const double d = (double)z[(long)i * dim] - mean;
            q += d * d;
        }
    const double var = col_sum(q, sm, ry, cx) / (n - 1);
    if (!ok) return;
    if (ry == 0) {
        mom[((long)view * 2 + 0) * dim + j] = mean;
        mom[((long)view * 2 + 1) * dim + j] = var;
    }
    float* a = v.a[view];
    float* c = v.c[view];
    if (a == nullptr && c == nullptr) return;
    const double sd = sqrt(var);                                   // no epsilon: a constant column divides by zero, as the reference
    for (int i = ry; i < n; i += BS_RL) {
        const double d = (double)z[(long)i * dim] - mean;
        if (a != nullptr) a[(long)i * dim + j] = (float)(d / sd);
        if (c != nullptr) c[(long)i * dim + j] = (float)d;
    }
}

// m [count, dim, dim]; partial [count, gridDim.x] (fp64)
__global__ void __launch_bounds__(256)
bs_matrix_pass_kernel(float* __restrict__ m, int dim, double inv_n, double target, double w_diag, double w_off,
                      double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const long per = (long)dim * dim;
    float* base = m + (long)blockIdx.y * per;
    const long i0 = (long)blockIdx.x * BS_PASS_CHUNK, i1 = min(per, i0 + BS_PASS_CHUNK);
    double acc = 0.0;
    for (long idx = i0 + threadIdx.x; idx < i1; idx += 256) {
        const long r = idx / dim, c = idx - r * dim;
        const double cv = (double)base[idx] * inv_n;
        double g = 0.0;
        if (r == c) {
            if (w_diag != 0.0) {
                const double e = cv - target;
                acc += w_diag * e * e;
                g = 2.0 * w_diag * e;
            }
        } else {
            acc += w_off * cv * cv;
            g = 2.0 * w_off * cv;
        }
        base[idx] = (float)g;
    }
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// loss = scale sum(partial) + var_w / dim sum over the variances of mom of relu(1 - sqrt(var + 1e-4))
__global__ void __launch_bounds__(256)
bs_finish_kernel(const double* __restrict__ partial, int n_partial, double scale, const double* __restrict__ mom, int views, int dim,
                 double var_w, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.0, hinge = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
    acc = block_sum_f64(acc, sm);
    if (var_w != 0.0) {
        for (int t = threadIdx.x; t < views * dim; t += 256) {
            const int view = t / dim, j = t - view * dim;
            const double h = 1.0 - sqrt(mom[((long)view * 2 + 1) * dim + j] + BS_VAR_EPS);
            if (h > 0.0) hinge += h;
        }
        hinge = block_sum_f64(hinge, sm);
    }
    if (threadIdx.x == 0) loss[0] = (float)(var_w != 0.0 ? acc * scale + hinge * (var_w / dim) : acc * scale);
}

__global__ void __launch_bounds__(256)
bs_col_bwd_kernel(BsBwd p, int n, int dim, const double* __restrict__ mom, double sa, double sc, double var_w, double gs,
                  const float* __restrict__ gs_dev) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[BS_RL][BS_CW];
    const int view = blockIdx.y, cx = threadIdx.x % BS_CW, ry = threadIdx.x / BS_CW;
    const int j = blockIdx.x * BS_CW + cx;
    const bool ok = j < dim;
    const long off = ok ? j : 0;
    const float* z = p.z[view];
    const float* a = p.a[view];
    const float* da = p.da[view];
    const float* dc = p.dc[view];
    if (gs_dev != nullptr) gs *= (double)gs_dev[0];                // the upstream scalar gradient stays on the device
    const double mean = ok ? mom[((long)view * 2 + 0) * dim + j] : 0.0;
    const double var = ok ? mom[((long)view * 2 + 1) * dim + j] : 1.0;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (da != nullptr) {                                           // (uniform over the workgroup)
        if (ok)
            for (int i = ry; i < n; i += BS_RL) {
                const double g = (double)da[(long)i * dim + off];
                s1 += g;
                s2 += g * (double)a[(long)i * dim + off];
            }
        s1 = col_sum(s1, sm, ry, cx) / n;
        s2 = col_sum(s2, sm, ry, cx) / (n - 1);
    }
    if (dc != nullptr) {
        if (ok)
            for (int i = ry; i < n; i += BS_RL) s3 += (double)dc[(long)i * dim + off];
        s3 = col_sum(s3, sm, ry, cx) / n;
    }
    if (!ok) return;
    const double inv_sd = 1.0 / sqrt(var);
    double hc = 0.0;
    if (var_w != 0.0) {
        const double sv = sqrt(var + BS_VAR_EPS);
        if (1.0 - sv > 0.0) hc = -var_w / ((double)dim * (n - 1) * sv);
    }
    float* dz = p.dz[view];
    for (int i = ry; i < n; i += BS_RL) {
        const long e = (long)i * dim + j;
        double v = 0.0;
        if (da != nullptr) v += sa * ((double)da[e] - s1 - (double)a[e] * s2) * inv_sd;
        if (dc != nullptr) v += sc * ((double)dc[e] - s3);
        if (hc != 0.0) v += hc * ((double)z[e] - mean);
        dz[e] = (float)(gs * v);
    }
}

// stats [rows, 1 + 2 reps] (fp64): |x|, |y_r|, <x, y_r>;  rowloss [rows] (fp64)
__global__ void __launch_bounds__(256)
bs_rows_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int dim, int reps, double* __restrict__ stats,
                   double* __restrict__ rowloss) {
    I3D_CHAIN_PRIO();
    __shared__ double sy[256], sd[256], sm[4], sinv[BS_MAX_REPS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nq = 256 / reps, span = nq * reps;                   // thread t < span keeps the repeat t % reps over its whole loop
    const bool active = t < span;
    const int q = t / reps;
    const float* xr = x + (long)b * dim;
    const float* yr = y + (long)b * dim * reps;
    const int total = dim * reps;
    double ax = 0.0;
    for (int d = t; d < dim; d += 256) ax += (double)xr[d] * (double)xr[d];
    ax = block_sum_f64(ax, sm);
    double ay = 0.0, ad = 0.0;
    if (active)
        for (int idx = t; idx < total; idx += span) {
            const double yv = (double)yr[idx];
            ay += yv * yv;
            ad += (double)xr[idx / reps] * yv;
        }
    sy[t] = ay;
    sd[t] = ad;
    for (int h = 128; h > 0; h >>= 1) {                            // over the threads of one repeat, a fixed tree
        __syncthreads();
        if (active && q < h && q + h < nq) {
            sy[t] += sy[t + h * reps];
            sd[t] += sd[t + h * reps];
        }
    }
    __syncthreads();
    const double nx = sqrt(ax);
    const double inx = 1.0 / fmax(nx, BS_NORM_EPS);
    double* st = stats + (long)b * (1 + 2 * reps);
    if (t < reps) {
        const double ny = sqrt(sy[t]);
        sinv[t] = 1.0 / fmax(ny, BS_NORM_EPS);
        st[1 + t] = ny;
        st[1 + reps + t] = sd[t];
    }
    if (t == 0) st[0] = nx;
    __syncthreads();
    double acc = 0.0;
    for (int idx = t; idx < total; idx += 256) {
        const int d = idx / reps, r = idx - d * reps;
        const double e = (double)xr[d] * inx - (double)yr[idx] * sinv[r];
        acc += e * e;
    }
    acc = block_sum_f64(acc, sm);
    if (t == 0) rowloss[b] = acc;
}

// k = grad_scale g;  x_hat = x / nx', y_hat_r = y_r / ny_r' (the clamped norms), c_r = <x_hat, y_hat_r>:
//     gx = k (reps x_hat - sum_r y_hat_r),  dx = (gx - x_hat <x_hat, gx>) / nx'      (|x| below the clamp: dx = gx / nx')
//     gy_r = -k (x_hat - y_hat_r),          dy_r = (gy_r - y_hat_r <y_hat_r, gy_r>) / ny_r'
__global__ void __launch_bounds__(256)
bs_rows_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int dim, int reps, const double* __restrict__ stats,
                   double k, const float* __restrict__ gs_dev, float* __restrict__ dx, float* __restrict__ dy) {
    I3D_CHAIN_PRIO();
    __shared__ double sinv[BS_MAX_REPS], sproj[BS_MAX_REPS], scr[BS_MAX_REPS];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* xr = x + (long)b * dim;
    const float* yr = y + (long)b * dim * reps;
    const double* st = stats + (long)b * (1 + 2 * reps);
    if (gs_dev != nullptr) k *= (double)gs_dev[0];
    const double nx = st[0];
    const double inx = 1.0 / fmax(nx, BS_NORM_EPS);
    const bool x_free = nx >= BS_NORM_EPS;                         // torch's clamp_min passes the gradient at equality
    if (t < reps) {
        const double ny = st[1 + t];
        const double iny = 1.0 / fmax(ny, BS_NORM_EPS);
        const double c = st[1 + reps + t] * inx * iny;
        const double yy = (ny * iny) * (ny * iny);
        sinv[t] = iny;
        scr[t] = c;
        sproj[t] = ny >= BS_NORM_EPS ? -k * (c - yy) : 0.0;        // <y_hat_r, gy_r>
    }
    __syncthreads();
    double csum = 0.0;
    for (int r = 0; r < reps; ++r) csum += scr[r];
    const double xx = (nx * inx) * (nx * inx);
    const double xproj = x_free ? k * (reps * xx - csum) : 0.0;    // <x_hat, gx>
    for (int d = t; d < dim; d += 256) {
        const double xh = (double)xr[d] * inx;
        double s = 0.0;
        for (int r = 0; r < reps; ++r) s += (double)yr[(long)d * reps + r] * sinv[r];
        const double gx = k * (reps * xh - s);
        dx[(long)b * dim + d] = (float)((gx - xh * xproj) * inx);
    }
    const int total = dim * reps;
    float* dyr = dy + (long)b * dim * reps;
    for (int idx = t; idx < total; idx += 256) {
        const int d = idx / reps, r = idx - d * reps;
        const double yh = (double)yr[idx] * sinv[r];
        const double gy = -k * ((double)xr[d] * inx - yh);
        dyr[idx] = (float)((gy - yh * sproj[r]) * sinv[r]);
    }
}

}  // namespace
}  // namespace i3d

using namespace i3d;

extern "C" int i3d_bs_max_repeats(void) { return BS_MAX_REPS; }

extern "C" int i3d_bs_pass_blocks(int dim) { return dim > 0 ? cdiv((long)dim * dim, BS_PASS_CHUNK) : 0; }

extern "C" int i3d_bs_moments(const float* z1, const float* z2, int n, int dim, float* a1, float* a2, float* c1, float* c2, double* mom,
                              void* stream) {
    I3D_CHECK_ARG(z1 != nullptr && mom != nullptr && dim > 0, "bad arguments");
    I3D_CHECK_ARG(n >= 2, "the unbiased variance needs two rows or more");
    I3D_CHECK_ARG(z2 != nullptr || (a2 == nullptr && c2 == nullptr), "outputs of a second view without the view");
    BsViews v;
    v.z[0] = z1; v.z[1] = z2;
    v.a[0] = a1; v.a[1] = a2;
    v.c[0] = c1; v.c[1] = c2;
    hipLaunchKernelGGL(bs_moments_kernel, dim3(cdiv(dim, BS_CW), z2 != nullptr ? 2 : 1), dim3(256), 0, (hipStream_t)stream, v, n, dim,
                       mom);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_bs_matrix_pass(float* m, int count, int dim, double inv_n, double target, double w_diag, double w_off,
                                  double* partial, void* stream) {
    I3D_CHECK_ARG(m != nullptr && partial != nullptr && dim > 0, "bad arguments");
    I3D_CHECK_ARG(count >= 1 && count <= 65535, "1..65535 matrices");
    hipLaunchKernelGGL(bs_matrix_pass_kernel, dim3(i3d_bs_pass_blocks(dim), count), dim3(256), 0, (hipStream_t)stream, m, dim, inv_n,
                       target, w_diag, w_off, partial);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_bs_finish(const double* partial, int n_partial, double scale, const double* mom, int views, int dim, double var_w,
                             float* loss, void* stream) {
    I3D_CHECK_ARG(loss != nullptr && n_partial >= 0 && (n_partial == 0 || partial != nullptr), "bad arguments");
    I3D_CHECK_ARG(var_w == 0.0 || (mom != nullptr && views >= 1 && views <= 2 && dim > 0), "the variance hinge needs the moments");
    hipLaunchKernelGGL(bs_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_partial, scale, mom, views, dim, var_w,
                       loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_bs_col_bwd(const float* z1, const float* z2, const float* a1, const float* a2, const float* da1, const float* da2,
                              const float* dc1, const float* dc2, int n, int dim, const double* mom, double sa, double sc, double var_w,
                              double grad_scale, const float* grad_scale_dev, float* dz1, float* dz2, void* stream) {
    I3D_CHECK_ARG(mom != nullptr && dz1 != nullptr && dim > 0, "bad arguments");
    I3D_CHECK_ARG(n >= 2, "the unbiased variance needs two rows or more");
    I3D_CHECK_ARG((da1 == nullptr || a1 != nullptr) && (da2 == nullptr || a2 != nullptr), "da without the standardised view");
    I3D_CHECK_ARG(var_w == 0.0 || (z1 != nullptr && (dz2 == nullptr || z2 != nullptr)), "the variance hinge needs z");
    I3D_CHECK_ARG(dz2 != nullptr || (da2 == nullptr && dc2 == nullptr), "gradients of a second view without dz2");
    BsBwd p;
    p.z[0] = z1; p.z[1] = z2;
    p.a[0] = a1; p.a[1] = a2;
    p.da[0] = da1; p.da[1] = da2;
    p.dc[0] = dc1; p.dc[1] = dc2;
    p.dz[0] = dz1; p.dz[1] = dz2;
    hipLaunchKernelGGL(bs_col_bwd_kernel, dim3(cdiv(dim, BS_CW), dz2 != nullptr ? 2 : 1), dim3(256), 0, (hipStream_t)stream, p, n, dim,
                       mom, sa, sc, var_w, grad_scale, grad_scale_dev);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_bs_rows_fwd(const float* x, const float* y, int rows, int dim, int reps, double* stats, double* rowloss,
                               void* stream) {
    I3D_CHECK_ARG(x != nullptr && y != nullptr && stats != nullptr && rowloss != nullptr && rows > 0 && dim > 0, "bad arguments");
    I3D_CHECK_ARG(reps >= 1 && reps <= BS_MAX_REPS, "repeats per row: 1..32");
    I3D_CHECK_ARG((long)dim * reps < (1L << 31) - 256, "a row of y too long");
    hipLaunchKernelGGL(bs_rows_fwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, y, dim, reps, stats, rowloss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_bs_rows_bwd(const float* x, const float* y, int rows, int dim, int reps, const double* stats, double grad_scale,
                               const float* grad_scale_dev, float* dx, float* dy, void* stream) {
    I3D_CHECK_ARG(x != nullptr && y != nullptr && stats != nullptr && dx != nullptr && dy != nullptr && rows > 0 && dim > 0,
                  "bad arguments");
    I3D_CHECK_ARG(reps >= 1 && reps <= BS_MAX_REPS, "repeats per row: 1..32");
    I3D_CHECK_ARG((long)dim * reps < (1L << 31) - 256, "a row of y too long");
    hipLaunchKernelGGL(bs_rows_bwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, y, dim, reps, stats, grad_scale,
                       grad_scale_dev, dx, dy);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
