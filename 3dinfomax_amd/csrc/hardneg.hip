// Single-positive contrastive losses that change how the negatives are weighted, forward and backward.
//
// Replaces the forward of InfoNCE (reference commons/losses.py:998-1034), InfoNCEHard (:1037-1074), NTXentHard (:1077-1114) and
// NTXentExtraNegatives (:889-943):
//     s'_ij = <z1_i, z2_j> / (|z1_i||z2_j|)  (no epsilon; norm == 0: the plain product),  P = exp(s'/tau),  p_i = pos_offset + i
//     pos_i = P[i, p_i],  S_i = sum_{j != p_i} P_ij,  A_i = sum_{j != p_i} P_ij^beta,  C_i = sum_{j != p_i} P_ij^(1 + beta)
//     InfoNCE               l_i = log(S_i + pos_i) - log pos_i
//     NTXentHard            Ng_i = (n C_i / A_i - tau_plus n pos_i) / (1 - tau_plus),  Ngc_i = max(Ng_i, n e^(-1/tau)),
//                           l_i = log Ngc_i - log pos_i                                             (n = b2 - 1)
//     InfoNCEHard           l_i = log(pos_i + Ngc_i) - log pos_i
//     NTXentExtraNegatives  l_i = log(S_i + w sum_u Q_iu) - log pos_i,  Q_iu = exp(<z1_i, x_iu> / (|z1_i||x_iu|) / tau)
// The shape is that of ntxent.hip: row norms (and the extra negatives' batched dots, one wave per (i, u)), the MFMA similarity GEMM, one
// fused row pass, the sum of the row losses; backward: one launch for dL/dsim and the norm-path terms, two GEMMs on top.  The row pass
// leaves four coefficients per row from which the backward forms dl_i/dP_ij P_ij with no further row statistics:
//     j == p_i: cp_i;   j != p_i: c1_i P_ij P_ij^beta + c2_i P_ij^beta  (P^beta = 1, c2 = 0 outside the hard modes);   extras: cq_i Q_iu
// The importance weights P^beta are differentiated through, as the reference's autograd does.  Row sums run in fp64 in a fixed order,
// no atomics: the same bits on every run.  Row-sharded like ntxent.hip: z1 are the local rows, z2 the gathered batch.
#include "common.h"

namespace i3d {
namespace {

constexpr int HN_INFONCE = 0, HN_NTXENT_HARD = 1, HN_INFONCE_HARD = 2, HN_EXTRA = 3;
constexpr int HN_MAX_EXTRA = 256;                 // extras per row: one pass of a row's workgroup
constexpr int HN_W = 8, HN_L = 32, HN_U = 8;      // column workgroups: 8 columns x 32 row lanes, rows 8 at a time

struct HnShape {
    int mode, b1, b2, n_extra, dim, pos_offset, norm;
    float inv_tau, beta;
};

struct HnRowMath {
    double n_neg, tau_plus, beta, floor, w;
};

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rows [0, b1): |z1_i|; [b1, b1 + b2): |z2_j|; then one wave per extra negative (i, u): <z1_i, x_iu> and |x_iu|.  norm == 0: ones.
template <bool VEC>
__global__ void __launch_bounds__(256)
hn_norms_kernel(const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ x, int b1, int b2, int n_extra,
                int dim, int norm, float* __restrict__ n1, float* __restrict__ n2, float* __restrict__ xdot, float* __restrict__ xn) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long total = (long)b1 + b2 + (long)b1 * n_extra;
    if (r >= total) return;
    if (r < b1 + b2) {
        float acc = 0.f;
        if (norm) {
            const float* z = r < b1 ? z1 + r * dim : z2 + (r - b1) * dim;
            if (VEC) {
                for (int c = lane * 4; c < dim; c += 256) {
                    const float4 v = *reinterpret_cast<const float4*>(z + c);
                    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
                }
            } else {
                for (int c = lane; c < dim; c += 64) acc += z[c] * z[c];
            }
            acc = wave_sum(acc);
        }
        if (lane == 0) {
            const float v = norm ? sqrtf(acc) : 1.f;
            if (r < b1) n1[r] = v;
            else n2[r - b1] = v;
        }
        return;
    }
    const long k = r - b1 - b2;
    const float* a = z1 + (k / n_extra) * dim;
    const float* e = x + k * dim;
    float dot = 0.f, sq = 0.f;
    if (VEC) {
        for (int c = lane * 4; c < dim; c += 256) {
            const float4 u = *reinterpret_cast<const float4*>(a + c);
            const float4 v = *reinterpret_cast<const float4*>(e + c);
            dot += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
            sq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int c = lane; c < dim; c += 64) {
            dot += a[c] * e[c];
            sq += e[c] * e[c];
        }
    }
    dot = wave_sum(dot);
    sq = wave_sum(sq);
    if (lane == 0) {
        xdot[k] = dot;
        xn[k] = norm ? sqrtf(sq) : 1.f;
    }
}

// dl_i/dP_ij P_ij of a negative from the row's coefficients
template <bool HARD>
__device__ __forceinline__ float hn_neg_term(float t, float c1, float c2, float beta) {
    const float p = expf(t);
    if (HARD) {
        const float pb = expf(beta * t);
        return c1 * (p * pb) + c2 * pb;
    }
    return c1 * p;
}

// stats [b1, 5] (fp64): pos, S, A, C (extra negatives: sum_u Q_iu in C's place), l;  coef [b1, 4]: cp, c1, c2, cq
template <bool HARD, bool VEC>
__global__ void __launch_bounds__(256)
hn_rows_fwd_kernel(HnShape sh, HnRowMath m, const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
                   const float* __restrict__ xdot, const float* __restrict__ xn, double* __restrict__ stats, float* __restrict__ coef) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int i = blockIdx.x, pcol = sh.pos_offset + i;
    const float a = n1[i];
    const float* row = sim + (long)i * sh.b2;
    double pos = 0.0, S = 0.0, A = 0.0, C = 0.0;
    auto element = [&](int j, float sv, float b) {
        const float t = sv / (a * b) * sh.inv_tau;
        const float p = expf(t);
        if (j == pcol) {
            pos = p;
        } else {
            S += p;
            if (HARD) {
                const float pb = expf(sh.beta * t);
                A += pb;
                C += p * pb;
            }
        }
    };
    if (VEC) {
        for (int j = threadIdx.x * 4; j < sh.b2; j += 1024) {
            const float4 sv = *reinterpret_cast<const float4*>(row + j);
            const float4 bv = *reinterpret_cast<const float4*>(n2 + j);
            element(j, sv.x, bv.x);
            element(j + 1, sv.y, bv.y);
            element(j + 2, sv.z, bv.z);
            element(j + 3, sv.w, bv.w);
        }
    } else {
        for (int j = threadIdx.x; j < sh.b2; j += 256) element(j, row[j], n2[j]);
    }
    if (sh.mode == HN_EXTRA) {
        for (int u = threadIdx.x; u < sh.n_extra; u += 256) {
            const long k = (long)i * sh.n_extra + u;
            C += expf(xdot[k] / (a * xn[k]) * sh.inv_tau);
        }
    }
    pos = block_sum_f64(pos, sm);
    S = block_sum_f64(S, sm);
    if (HARD) A = block_sum_f64(A, sm);
    if (HARD || sh.mode == HN_EXTRA) C = block_sum_f64(C, sm);
    if (threadIdx.x != 0) return;
    double l, cp, c1, c2 = 0.0, cq = 0.0;
    if (sh.mode == HN_INFONCE) {
        const double den = S + pos;
        l = log(den) - log(pos);
        c1 = 1.0 / den;
        cp = pos / den - 1.0;
    } else if (sh.mode == HN_EXTRA) {
        const double den = S + m.w * C;
        l = log(den) - log(pos);
        c1 = 1.0 / den;
        cp = -1.0;
        cq = m.w / den;
    } else {
        const double ng = (m.n_neg * C / A - m.tau_plus * m.n_neg * pos) / (1.0 - m.tau_plus);
        const double k = ng >= m.floor ? 1.0 : 0.0;            // torch.clamp passes the gradient at equality
        const double ngc = ng >= m.floor ? ng : m.floor;
        const double den = sh.mode == HN_INFONCE_HARD ? pos + ngc : ngc;
        const double q = 1.0 / den;
        l = log(den) - log(pos);
        const double f = q * k * m.n_neg / (1.0 - m.tau_plus);
        cp = pos * ((sh.mode == HN_INFONCE_HARD ? q : 0.0) - f * m.tau_plus) - 1.0;
        c1 = f * (1.0 + m.beta) / A;
        c2 = -f * m.beta * C / (A * A);
    }
    double* st = stats + (long)i * 5;
    st[0] = pos; st[1] = S; st[2] = A; st[3] = C; st[4] = l;
    *reinterpret_cast<float4*>(coef + (long)i * 4) = make_float4((float)cp, (float)c1, (float)c2, (float)cq);
}

__global__ void __launch_bounds__(256)
hn_loss_kernel(const double* __restrict__ stats, int b1, double scale, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < b1; i += 256) acc += stats[(long)i * 5 + 4];
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(acc * scale);
}

// G_ij = gs / tau * dl_i/dP_ij P_ij.  Workgroups [0, b1) are the rows: dsim_ij = G_ij / (a_i b_j), ca_i = -(1 / a_i^2) sum_j G_ij s'_ij
// (the extra negatives' terms included), dz1_i = ca_i z1_i + sum_u H_iu x_iu and dx_iu = H_iu z1_i - T_iu x_iu with
// H_iu = G_iu / (a_i |x_iu|), T_iu = G_iu s'_iu / |x_iu|^2.  The rest take HN_W columns each: cb_j = -(1 / b_j^2) sum_i G_ij s'_ij from
// sim and the rows' coefficients (the same G_ij, recomputed), dz2_j = cb_j z2_j.  The two GEMMs behind it accumulate dS z2 and dS^T z1.
template <bool HARD, bool VEC>
__global__ void __launch_bounds__(256)
hn_bwd_kernel(HnShape sh, const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
              const float* __restrict__ coef, const float* __restrict__ xdot, const float* __restrict__ xn,
              const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ x, float gs,
              const float* __restrict__ gs_dev, float* __restrict__ dsim, float* __restrict__ ca_out, float* __restrict__ cb_out,
              float* __restrict__ dz1, float* __restrict__ dz2, float* __restrict__ dx) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[HN_L][HN_W];
    __shared__ float sH[HN_MAX_EXTRA], sT[HN_MAX_EXTRA];
    __shared__ float cbs[HN_W];
    if (gs_dev != nullptr) gs *= gs_dev[0];      // the upstream scalar gradient stays on the device
    const float gt = gs * sh.inv_tau;
    if ((int)blockIdx.x < sh.b1) {
        const int i = blockIdx.x, pcol = sh.pos_offset + i;
        const float a = n1[i];
        const float4 cf = *reinterpret_cast<const float4*>(coef + (long)i * 4);
        const float* row = sim + (long)i * sh.b2;
        float* drow = dsim + (long)i * sh.b2;
        double da = 0.0;
        auto element = [&](int j, float sv, float b) -> float {
            const float nrm = a * b;
            const float s = sv / nrm;
            const float G = gt * (j == pcol ? cf.x : hn_neg_term<HARD>(s * sh.inv_tau, cf.y, cf.z, sh.beta));
            da += G * s;
            return G / nrm;
        };
        if (VEC) {
            for (int j = threadIdx.x * 4; j < sh.b2; j += 1024) {
                const float4 sv = *reinterpret_cast<const float4*>(row + j);
                const float4 bv = *reinterpret_cast<const float4*>(n2 + j);
                float4 o;
                o.x = element(j, sv.x, bv.x);
                o.y = element(j + 1, sv.y, bv.y);
                o.z = element(j + 2, sv.z, bv.z);
                o.w = element(j + 3, sv.w, bv.w);
                *reinterpret_cast<float4*>(drow + j) = o;
            }
        } else {
            for (int j = threadIdx.x; j < sh.b2; j += 256) drow[j] = element(j, row[j], n2[j]);
        }
        const long k0 = (long)i * sh.n_extra;
        if ((int)threadIdx.x < sh.n_extra) {                     // n_extra <= HN_MAX_EXTRA = the workgroup's size
            const float e = xn[k0 + threadIdx.x];
            const float s = xdot[k0 + threadIdx.x] / (a * e);
            const float G = gt * cf.w * expf(s * sh.inv_tau);
            sH[threadIdx.x] = G / (a * e);
            sT[threadIdx.x] = sh.norm ? G * s / (e * e) : 0.f;
            da += G * s;
        }
        da = block_sum_f64(da, &sm[0][0]);                       // (its barriers publish sH and sT)
        const float ca = (sh.norm && a > 0.f) ? (float)(-da / ((double)a * a)) : 0.f;
        if (threadIdx.x == 0 && ca_out != nullptr) ca_out[i] = ca;
        if (dz1 == nullptr) return;
        const float* zi = z1 + (long)i * sh.dim;
        for (int c = threadIdx.x; c < sh.dim; c += 256) {
            const float zv = zi[c];
            float v = ca * zv;
            for (int u = 0; u < sh.n_extra; ++u) {
                const float xv = x[(k0 + u) * sh.dim + c];
                v += sH[u] * xv;
                dx[(k0 + u) * sh.dim + c] = sH[u] * zv - sT[u] * xv;
            }
            dz1[(long)i * sh.dim + c] = v;
        }
        return;
    }
    const int j0 = ((int)blockIdx.x - sh.b1) * HN_W;
    const int cx = threadIdx.x % HN_W, ry = threadIdx.x / HN_W;
    const int j = j0 + cx;
    const bool col_ok = j < sh.b2;
    const float b = col_ok ? n2[j] : 1.f;
    double acc = 0.0;
    if (sh.norm) {
        for (int i0 = ry; i0 < sh.b1; i0 += HN_L * HN_U) {
            float sv[HN_U], av[HN_U];
            float4 cv[HN_U];
#pragma unroll
            for (int u = 0; u < HN_U; ++u) {                     // the loads of a group in flight together
                const int i = i0 + u * HN_L;
                const bool ok = col_ok && i < sh.b1;
                sv[u] = ok ? sim[(long)i * sh.b2 + j] : 0.f;
                av[u] = ok ? n1[i] : 1.f;
                cv[u] = ok ? *reinterpret_cast<const float4*>(coef + (long)i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < HN_U; ++u) {
                const int i = i0 + u * HN_L;
                const float s = sv[u] / (av[u] * b);
                const float G = gt * (j == sh.pos_offset + i ? cv[u].x : hn_neg_term<HARD>(s * sh.inv_tau, cv[u].y, cv[u].z, sh.beta));
                if (col_ok && i < sh.b1) acc += G * s;
            }
        }
    }
    sm[ry][cx] = acc;
    __syncthreads();
    if (ry == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < HN_L; ++k) t += sm[k][cx];
        const float cb = (sh.norm && col_ok && b > 0.f) ? (float)(-t / ((double)b * b)) : 0.f;
        cbs[cx] = cb;
        if (col_ok && cb_out != nullptr) cb_out[j] = cb;
    }
    __syncthreads();
    if (dz2 == nullptr) return;
    const int items = min(HN_W, sh.b2 - j0) * sh.dim;
    for (int t = threadIdx.x; t < items; t += 256) dz2[(long)j0 * sh.dim + t] = cbs[t / sh.dim] * z2[(long)j0 * sh.dim + t];
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline long al4(long n) { return (n + 3) & ~3L; }
inline bool hard_mode(int mode) { return mode == HN_NTXENT_HARD || mode == HN_INFONCE_HARD; }

struct HnScratch {
    float *n1, *n2, *coef, *xdot, *xn, *sim;
    double* stats;
    long floats;
};

// n1[b1] | n2[b2] | coef[4 b1] | stats[5 b1] (fp64) | xdot[b1 U] | xn[b1 U] | sim[b1, b2], every part 16-byte aligned
HnScratch hn_scratch(float* base, int b1, int b2, int n_extra) {
    const long o_n2 = al4(b1), o_coef = o_n2 + al4(b2), o_stats = o_coef + 4L * b1, o_xdot = o_stats + al4(10L * b1);
    const long o_xn = o_xdot + al4((long)b1 * n_extra), o_sim = o_xn + al4((long)b1 * n_extra);
    HnScratch s = {};
    s.floats = o_sim + al4((long)b1 * b2);
    if (base == nullptr) return s;
    s.n1 = base;
    s.n2 = base + o_n2;
    s.coef = base + o_coef;
    s.stats = reinterpret_cast<double*>(base + o_stats);
    s.xdot = base + o_xdot;
    s.xn = base + o_xn;
    s.sim = base + o_sim;
    return s;
}

int hn_check(const char* who, int mode, int b1, int b2, int n_extra, int pos_offset, double tau, double tau_plus) {
    auto bad = [&](const char* msg) {
        set_error("%s: invalid argument: %s", who, msg);
        return I3D_ERR_INVALID;
    };
    if (mode < HN_INFONCE || mode > HN_EXTRA) return bad("mode is 0 (InfoNCE), 1 (NTXentHard), 2 (InfoNCEHard) or 3 (NTXentExtraNegatives)");
    if (b1 < 1 || b2 < 1) return bad("bad shape");
    if (!(tau > 0.0)) return bad("tau must be positive");
    if (pos_offset < 0 || (long)pos_offset + b1 > b2) return bad("positive columns out of range");
    if (hard_mode(mode) && b2 < 2) return bad("the hard-negative losses need two columns or more: a batch of one has no negatives");
    if (hard_mode(mode) && !(tau_plus < 1.0)) return bad("tau_plus must be below 1");
    if (mode == HN_EXTRA ? (n_extra < 0 || n_extra > HN_MAX_EXTRA) : n_extra != 0)
        return bad("extra negatives per row: 0..256 for mode 3, none for the other modes");
    return I3D_OK;
}

HnShape hn_shape(int mode, int b1, int b2, int n_extra, int dim, int pos_offset, int norm, double tau, double beta) {
    HnShape sh;
    sh.mode = mode; sh.b1 = b1; sh.b2 = b2; sh.n_extra = n_extra; sh.dim = dim; sh.pos_offset = pos_offset; sh.norm = norm;
    sh.inv_tau = (float)(1.0 / tau);
    sh.beta = (float)beta;
    return sh;
}

}  // namespace
}  // namespace i3d

using namespace i3d;

extern "C" int i3d_hardneg_max_extra(void) { return HN_MAX_EXTRA; }

extern "C" int i3d_hardneg_norms(const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim, int norm,
                                 float* n1, float* n2, float* xdot, float* xn, void* stream) {
    I3D_CHECK_ARG(z1 != nullptr && z2 != nullptr && n1 != nullptr && n2 != nullptr && b1 > 0 && b2 > 0 && dim > 0, "bad arguments");
    I3D_CHECK_ARG(n_extra >= 0 && n_extra <= HN_MAX_EXTRA, "extra negatives per row: 0..256");
    I3D_CHECK_ARG(n_extra == 0 || (x != nullptr && xdot != nullptr && xn != nullptr), "extra negatives without their buffers");
    const long rows = (long)b1 + b2 + (long)b1 * n_extra;
    I3D_CHECK_ARG(rows < (1L << 31) - 4, "too many rows");
    const bool vec = dim % 4 == 0 && aligned16(z1) && aligned16(z2) && (n_extra == 0 || aligned16(x));
    auto kernel = vec ? hn_norms_kernel<true> : hn_norms_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, z1, z2, x, b1, b2, n_extra, dim, norm, n1, n2,
                       xdot, xn);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_hardneg_fwd(int mode, const float* sim, const float* n1, const float* n2, const float* xdot, const float* xn, int b1,
                               int b2, int n_extra, int pos_offset, double tau, double tau_plus, double beta, double extra_weight,
                               double loss_scale, double* stats, float* coef, float* loss, void* stream) {
    int rc;
    if ((rc = hn_check(__func__, mode, b1, b2, n_extra, pos_offset, tau, tau_plus)) != I3D_OK) return rc;
    I3D_CHECK_ARG(sim != nullptr && n1 != nullptr && n2 != nullptr && stats != nullptr && coef != nullptr && loss != nullptr, "null");
    I3D_CHECK_ARG(n_extra == 0 || (xdot != nullptr && xn != nullptr), "extra negatives without their buffers");
    I3D_CHECK_ARG(aligned16(coef) && aligned16(stats), "coef and stats must be 16-byte aligned");
    const HnShape sh = hn_shape(mode, b1, b2, n_extra, 0, pos_offset, 1, tau, beta);
    HnRowMath m;
    m.n_neg = (double)(b2 - 1);
    m.tau_plus = tau_plus;
    m.beta = beta;
    m.floor = m.n_neg * exp(-1.0 / tau);
    m.w = extra_weight;
    const bool vec = b2 % 4 == 0 && aligned16(sim) && aligned16(n2);
    const bool hard = hard_mode(mode);
    auto kernel = hard ? (vec ? hn_rows_fwd_kernel<true, true> : hn_rows_fwd_kernel<true, false>)
                       : (vec ? hn_rows_fwd_kernel<false, true> : hn_rows_fwd_kernel<false, false>);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kernel, dim3(b1), dim3(256), 0, s, sh, m, sim, n1, n2, xdot, xn, stats, coef);
    I3D_CHECK_LAUNCH();
    // the rows' kernel and the one-workgroup sum stay two launches, as in i3d_ntxent_loss_fwd
    hipLaunchKernelGGL(hn_loss_kernel, dim3(1), dim3(256), 0, s, stats, b1, loss_scale, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_hardneg_bwd(int mode, const float* sim, const float* n1, const float* n2, const float* coef, const float* xdot,
                               const float* xn, const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim,
                               int pos_offset, int norm, double tau, double beta, double grad_scale, const float* grad_scale_dev,
                               float* dsim, float* ca, float* cb, float* dz1, float* dz2, float* dx, void* stream) {
    int rc;
    if ((rc = hn_check(__func__, mode, b1, b2, n_extra, pos_offset, tau, 0.0)) != I3D_OK) return rc;
    I3D_CHECK_ARG(sim != nullptr && n1 != nullptr && n2 != nullptr && coef != nullptr && dsim != nullptr, "null");
    I3D_CHECK_ARG(aligned16(coef), "coef must be 16-byte aligned");
    I3D_CHECK_ARG((dz1 == nullptr) == (dz2 == nullptr), "dz1 and dz2 come together");
    I3D_CHECK_ARG(dz1 == nullptr || (z1 != nullptr && z2 != nullptr && dim > 0), "dz1 and dz2 need z1, z2 and dim");
    I3D_CHECK_ARG(n_extra == 0 || (xdot != nullptr && xn != nullptr), "extra negatives without their buffers");
    I3D_CHECK_ARG(n_extra == 0 || dz1 == nullptr || (x != nullptr && dx != nullptr), "extra negatives without x and dx");
    const HnShape sh = hn_shape(mode, b1, b2, n_extra, dim, pos_offset, norm, tau, beta);
    const bool vec = b2 % 4 == 0 && aligned16(sim) && aligned16(n2) && aligned16(dsim);
    const bool hard = hard_mode(mode);
    auto kernel = hard ? (vec ? hn_bwd_kernel<true, true> : hn_bwd_kernel<true, false>)
                       : (vec ? hn_bwd_kernel<false, true> : hn_bwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(b1 + cdiv(b2, HN_W)), dim3(256), 0, (hipStream_t)stream, sh, sim, n1, n2, coef, xdot, xn, z1, z2, x,
                       (float)grad_scale, grad_scale_dev, dsim, ca, cb, dz1, dz2, dx);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

// ---- the whole loss from one C call per direction (host sequencing only: the kernels above + the similarity GEMMs) ----
extern "C" long i3d_hardneg_loss_scratch_floats(int b1, int b2, int n_extra) {
    if (b1 < 1 || b2 < 1 || n_extra < 0) return 0;
    return hn_scratch(nullptr, b1, b2, n_extra).floats;
}

extern "C" int i3d_hardneg_loss_fwd(int mode, const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim,
                                    int pos_offset, int norm, double tau, double tau_plus, double beta, double extra_weight,
                                    double loss_scale, float* scratch, float* loss, void* stream) {
    int rc;
    if ((rc = hn_check(__func__, mode, b1, b2, n_extra, pos_offset, tau, tau_plus)) != I3D_OK) return rc;
    I3D_CHECK_ARG(z1 != nullptr && z2 != nullptr && scratch != nullptr && loss != nullptr && dim > 0, "bad arguments");
    I3D_CHECK_ARG(aligned16(scratch), "scratch must be 16-byte aligned");
    const HnScratch s = hn_scratch(scratch, b1, b2, n_extra);
    if ((rc = i3d_hardneg_norms(z1, z2, x, b1, b2, n_extra, dim, norm, s.n1, s.n2, s.xdot, s.xn, stream)) != I3D_OK) return rc;
    if ((rc = i3d_gemm_f32(0, 1, b1, b2, dim, z1, dim, z2, dim, s.sim, b2, nullptr, 0, stream)) != I3D_OK) return rc;
    return i3d_hardneg_fwd(mode, s.sim, s.n1, s.n2, s.xdot, s.xn, b1, b2, n_extra, pos_offset, tau, tau_plus, beta, extra_weight,
                           loss_scale, s.stats, s.coef, loss, stream);
}

// dz1 [b1, dim], dz2 [b2, dim], dx [b1 n_extra, dim]; work: b1 * b2 floats, 16-byte aligned (dL/dsim)
extern "C" int i3d_hardneg_loss_bwd(int mode, const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim,
                                    int pos_offset, int norm, double tau, double beta, double loss_scale, const float* scratch,
                                    const float* grad_scale_dev, float* work, float* dz1, float* dz2, float* dx, void* stream) {
    I3D_CHECK_ARG(z1 != nullptr && z2 != nullptr && scratch != nullptr && work != nullptr && dz1 != nullptr && dz2 != nullptr && dim > 0,
                  "bad arguments");
    I3D_CHECK_ARG(b1 > 0 && b2 > 0 && n_extra >= 0, "bad shape");
    const HnScratch s = hn_scratch(const_cast<float*>(scratch), b1, b2, n_extra);
    int rc;
    if ((rc = i3d_hardneg_bwd(mode, s.sim, s.n1, s.n2, s.coef, s.xdot, s.xn, z1, z2, x, b1, b2, n_extra, dim, pos_offset, norm, tau, beta,
                              loss_scale, grad_scale_dev, work, nullptr, nullptr, dz1, dz2, dx, stream)) != I3D_OK) return rc;
    if ((rc = i3d_gemm_f32(0, 0, b1, dim, b2, work, b2, z2, dim, dz1, dim, nullptr, 1, stream)) != I3D_OK) return rc;
    return i3d_gemm_f32(1, 0, b2, dim, b1, work, b2, z1, dim, dz2, dim, nullptr, 1, stream);
}
