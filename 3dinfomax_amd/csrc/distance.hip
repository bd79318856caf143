// Kernels of the distance-prediction baseline (reference models/distance_predictor.py): the per-molecule multi-head
// self-attention of its TransformerEncoderLayer, LayerNorm with the residual add fused, and the pair head over the
// complete graph's ordered atom pairs.  fp32, deterministic: every sum runs in a fixed order inside one workgroup or
// through per-block partials reduced in block order; no float atomics.
//
// Attention layout: the molecules of a batch are contiguous node ranges [graph_ptr[g], graph_ptr[g+1]) ("compact" order,
// no padding).  qkv is the [N, 3H] output of the in_proj product (q | k | v, head h at columns h*dh .. h*dh+dh-1 of each
// third, torch.nn.MultiheadAttention's split).  One workgroup per (molecule, head), four waves; each wave owns one query
// row at a time and streams the molecule's keys through LDS in tiles of ATT_KT with an online softmax, so a molecule of
// any size runs in the same LDS.  Inside a tile, lane (k, half) computes half of the dot product of key k (the two halves
// meet through one cross-lane add: both lanes hold the same sum), the P.V product has the head dimension on the lanes.
#include "common.h"

namespace i3d {

constexpr int ATT_KT = 32;          // keys (forward, dQ pass) / queries (dK-dV pass) per LDS tile
constexpr int ATT_WAVES = 4;
constexpr int ATT_MAX_DH = 128;     // head width: at most 2 values per lane
constexpr int LN_ROWS = 32;         // rows per workgroup of the LayerNorm backward (one block of column partials)

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // xor butterfly: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// half-wave dot product over [0, dh): lanes 0-31 take dims [0, split), lanes 32-63 dims [split, dh); a and b row pointers
// of the lane's own rows; the result is the full sum in both lanes of the pair (k, k + 32)
__device__ __forceinline__ float half_dot(const float* a, const float* b, int dh, int half) {
    const int split = (dh + 1) >> 1;
    const int d0 = half ? split : 0, d1 = half ? dh : split;
    float s = 0.f;
    for (int d = d0; d < d1; ++d) s += a[d] * b[d];
    return s + __shfl_xor(s, 32);
}

// rows [r0, r0 + cnt) of the column block [col, col + dh) of a row-major matrix with leading dimension ld -> LDS [cnt][ldl]
__device__ __forceinline__ void stage_rows(float* dst, int ldl, const float* src, long ld, int col, int r0, int cnt, int dh) {
    for (int e = threadIdx.x; e < cnt * dh; e += blockDim.x) {
        const int r = e / dh, d = e - r * dh;
        dst[r * ldl + d] = src[(long)(r0 + r) * ld + col + d];
    }
}

template <int DPL>
__global__ void __launch_bounds__(256)
mha_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ graph_ptr, int H, int nhead, int dh, float scale,
               float* __restrict__ out, float* __restrict__ lse) {
    I3D_CHAIN_PRIO();
    extern __shared__ float smem[];
    const int ldk = dh + 1;
    float* Ks = smem;                       // [KT][dh + 1]
    float* Vs = Ks + ATT_KT * ldk;          // [KT][dh]
    float* Qs = Vs + ATT_KT * dh;           // [WAVES][dh]
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, kl = lane & 31;
    const long ld = 3L * H;
    const int qc = hd * dh, kc = H + hd * dh, vc = 2 * H + hd * dh;
    const bool single = n <= ATT_KT;        // the whole molecule is one tile: staged once
    if (single) {
        stage_rows(Ks, ldk, qkv, ld, kc, n0, n, dh);
        stage_rows(Vs, dh, qkv, ld, vc, n0, n, dh);
    }
    for (int q0 = 0; q0 < n; q0 += ATT_WAVES) {
        const int qi = q0 + w;
        const bool active = qi < n;
        __syncthreads();                    // the previous rows' readers of Qs are done
        if (active)
            for (int d = lane; d < dh; d += 64) Qs[w * dh + d] = qkv[(long)(n0 + qi) * ld + qc + d];
        float m = -INFINITY, l = 0.f, o[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) o[c] = 0.f;
        for (int k0 = 0; k0 < n; k0 += ATT_KT) {
            const int kt = min(ATT_KT, n - k0);
            if (!single) {
                __syncthreads();
                stage_rows(Ks, ldk, qkv, ld, kc, n0 + k0, kt, dh);
                stage_rows(Vs, dh, qkv, ld, vc, n0 + k0, kt, dh);
            }
            __syncthreads();
            if (!active) continue;
            const float dot = half_dot(Qs + w * dh, Ks + (kl < kt ? kl : 0) * ldk, dh, half);
            const float s = kl < kt ? dot * scale : -INFINITY;
            const float m_new = fmaxf(m, wave_max(s));
            const float p = kl < kt ? expf(s - m_new) : 0.f;
            const float corr = expf(m - m_new);             // 0 on the first tile (m = -inf)
            l = l * corr + wave_sum(half ? 0.f : p);
            m = m_new;
#pragma unroll
            for (int c = 0; c < DPL; ++c) o[c] *= corr;
            for (int j = 0; j < kt; ++j) {
                const float pj = __shfl(p, j);
#pragma unroll
                for (int c = 0; c < DPL; ++c) {
                    const int d = lane + 64 * c;
                    if (d < dh) o[c] += pj * Vs[j * dh + d];
                }
            }
        }
        if (active) {
            const float inv = 1.f / l;
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                const int d = lane + 64 * c;
                if (d < dh) out[(long)(n0 + qi) * H + qc + d] = o[c] * inv;
            }
            if (lane == 0) lse[(long)(n0 + qi) * nhead + hd] = m + logf(l);
        }
    }
}

// backward, pass 1 (query rows on the waves): delta_i = dO_i . O_i, dQ_i = scale * sum_j P_ij (dP_ij - delta_i) K_j with
// P_ij = exp(scale q_i.k_j - lse_i) recomputed and dP_ij = dO_i . v_j
template <int DPL>
__global__ void __launch_bounds__(256)
mha_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ o_, const float* __restrict__ dout,
                  const float* __restrict__ lse, const int* __restrict__ graph_ptr, int H, int nhead, int dh, float scale,
                  float* __restrict__ delta, float* __restrict__ dqkv) {
    I3D_CHAIN_PRIO();
    extern __shared__ float smem[];
    const int ldk = dh + 1;
    float* Ks = smem;                       // [KT][dh + 1]
    float* Vs = Ks + ATT_KT * ldk;          // [KT][dh + 1]
    float* Qs = Vs + ATT_KT * ldk;          // [WAVES][dh]
    float* dOs = Qs + ATT_WAVES * dh;       // [WAVES][dh]
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, kl = lane & 31;
    const long ld = 3L * H;
    const int qc = hd * dh, kc = H + hd * dh, vc = 2 * H + hd * dh;
    const bool single = n <= ATT_KT;
    if (single) {
        stage_rows(Ks, ldk, qkv, ld, kc, n0, n, dh);
        stage_rows(Vs, ldk, qkv, ld, vc, n0, n, dh);
    }
    for (int q0 = 0; q0 < n; q0 += ATT_WAVES) {
        const int qi = q0 + w;
        const bool active = qi < n;
        const long row = n0 + qi;
        __syncthreads();
        float dl = 0.f, L = 0.f;
        if (active) {
            float part = 0.f;
            for (int d = lane; d < dh; d += 64) {
                const float gq = dout[row * H + qc + d];
                Qs[w * dh + d] = qkv[row * ld + qc + d];
                dOs[w * dh + d] = gq;
                part += gq * o_[row * H + qc + d];
            }
            dl = wave_sum(part);
            L = lse[row * nhead + hd];
            if (lane == 0) delta[row * nhead + hd] = dl;
        }
        float dq[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) dq[c] = 0.f;
        for (int k0 = 0; k0 < n; k0 += ATT_KT) {
            const int kt = min(ATT_KT, n - k0);
            if (!single) {
                __syncthreads();
                stage_rows(Ks, ldk, qkv, ld, kc, n0 + k0, kt, dh);
                stage_rows(Vs, ldk, qkv, ld, vc, n0 + k0, kt, dh);
            }
            __syncthreads();
            if (!active) continue;
            const int kr = kl < kt ? kl : 0;
            const float s = half_dot(Qs + w * dh, Ks + kr * ldk, dh, half) * scale;
            const float dp = half_dot(dOs + w * dh, Vs + kr * ldk, dh, half);
            const float ds = kl < kt ? expf(s - L) * (dp - dl) : 0.f;
            for (int j = 0; j < kt; ++j) {
                const float dsj = __shfl(ds, j);
#pragma unroll
                for (int c = 0; c < DPL; ++c) {
                    const int d = lane + 64 * c;
                    if (d < dh) dq[c] += dsj * Ks[j * ldk + d];
                }
            }
        }
        if (active) {
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                const int d = lane + 64 * c;
                if (d < dh) dqkv[row * ld + qc + d] = dq[c] * scale;
            }
        }
    }
}

// backward, pass 2 (key rows on the waves): dV_j = sum_i P_ij dO_i, dK_j = scale * sum_i P_ij (dP_ij - delta_i) Q_i
template <int DPL>
__global__ void __launch_bounds__(256)
mha_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                   const float* __restrict__ delta, const int* __restrict__ graph_ptr, int H, int nhead, int dh, float scale,
                   float* __restrict__ dqkv) {
    I3D_CHAIN_PRIO();
    extern __shared__ float smem[];
    const int ldk = dh + 1;
    float* Qs = smem;                       // [KT][dh + 1]   query tile
    float* dOs = Qs + ATT_KT * ldk;         // [KT][dh + 1]
    float* Kw = dOs + ATT_KT * ldk;         // [WAVES][dh]    the wave's key row
    float* Vw = Kw + ATT_WAVES * dh;        // [WAVES][dh]
    float* Ls = Vw + ATT_WAVES * dh;        // [KT] lse of the tile's queries
    float* Ds = Ls + ATT_KT;                // [KT] delta
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = graph_ptr[g], n = graph_ptr[g + 1] - n0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, il = lane & 31;
    const long ld = 3L * H;
    const int qc = hd * dh, kc = H + hd * dh, vc = 2 * H + hd * dh;
    const bool single = n <= ATT_KT;
    auto stage_queries = [&](int i0, int it) {
        stage_rows(Qs, ldk, qkv, ld, qc, n0 + i0, it, dh);
        stage_rows(dOs, ldk, dout, H, qc, n0 + i0, it, dh);
        for (int e = threadIdx.x; e < it; e += blockDim.x) {
            Ls[e] = lse[(long)(n0 + i0 + e) * nhead + hd];
            Ds[e] = delta[(long)(n0 + i0 + e) * nhead + hd];
        }
    };
    if (single) stage_queries(0, n);
    for (int j0 = 0; j0 < n; j0 += ATT_WAVES) {
        const int kj = j0 + w;
        const bool active = kj < n;
        const long row = n0 + kj;
        __syncthreads();
        if (active)
            for (int d = lane; d < dh; d += 64) {
                Kw[w * dh + d] = qkv[row * ld + kc + d];
                Vw[w * dh + d] = qkv[row * ld + vc + d];
            }
        float dk[DPL], dv[DPL];
#pragma unroll
        for (int c = 0; c < DPL; ++c) dk[c] = dv[c] = 0.f;
        for (int i0 = 0; i0 < n; i0 += ATT_KT) {
            const int it = min(ATT_KT, n - i0);
            if (!single) {
                __syncthreads();
                stage_queries(i0, it);
            }
            __syncthreads();
            if (!active) continue;
            const int ir = il < it ? il : 0;
            const float s = half_dot(Qs + ir * ldk, Kw + w * dh, dh, half) * scale;
            const float dp = half_dot(dOs + ir * ldk, Vw + w * dh, dh, half);
            const float p = il < it ? expf(s - Ls[ir]) : 0.f;
            const float ds = il < it ? p * (dp - Ds[ir]) : 0.f;
            for (int i = 0; i < it; ++i) {
                const float pi = __shfl(p, i), dsi = __shfl(ds, i);
#pragma unroll
                for (int c = 0; c < DPL; ++c) {
                    const int d = lane + 64 * c;
                    if (d < dh) {
                        dv[c] += pi * dOs[i * ldk + d];
                        dk[c] += dsi * Qs[i * ldk + d];
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int c = 0; c < DPL; ++c) {
                const int d = lane + 64 * c;
                if (d < dh) {
                    dqkv[row * ld + kc + d] = dk[c] * scale;
                    dqkv[row * ld + vc + d] = dv[c];
                }
            }
        }
    }
}

// ---- LayerNorm of (x + r): one wave per row ------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
ln_res_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ gamma,
                  const float* __restrict__ beta, int rows, int feat, float eps, float* __restrict__ y,
                  float* __restrict__ mean, float* __restrict__ rstd) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * feat;
    const float* rr = r + row * feat;
    float s = 0.f;
    for (int c = lane; c < feat; c += 64) s += xr[c] + rr[c];
    const float mu = wave_sum(s) / (float)feat;
    float v = 0.f;
    for (int c = lane; c < feat; c += 64) {
        const float z = (xr[c] + rr[c]) - mu;
        v += z * z;
    }
    const float rs = 1.f / sqrtf(wave_sum(v) / (float)feat + eps);
    for (int c = lane; c < feat; c += 64) y[row * feat + c] = ((xr[c] + rr[c]) - mu) * rs * gamma[c] + beta[c];
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

// dz = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; per block of LN_ROWS rows the column partials
// sum(dy xhat) and sum(dy) (rows in order), reduced over the blocks in order by ln_colreduce_kernel
__global__ void __launch_bounds__(256)
ln_res_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ r,
                  const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd, int rows,
                  int feat, float* __restrict__ dz, float* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r0 = blockIdx.x * LN_ROWS, r1 = min(rows, r0 + LN_ROWS);
    for (int row = r0 + w; row < r1; row += 4) {
        const long o = (long)row * feat;
        const float mu = mean[row], rs = rstd[row];
        float a = 0.f, b = 0.f;
        for (int c = lane; c < feat; c += 64) {
            const float gc = dy[o + c] * gamma[c];
            a += gc;
            b += gc * (((x[o + c] + r[o + c]) - mu) * rs);
        }
        a = wave_sum(a) / (float)feat;
        b = wave_sum(b) / (float)feat;
        for (int c = lane; c < feat; c += 64) {
            const float xh = ((x[o + c] + r[o + c]) - mu) * rs;
            dz[o + c] = rs * (dy[o + c] * gamma[c] - a - xh * b);
        }
    }
    for (int c = threadIdx.x; c < feat; c += blockDim.x) {
        float sg = 0.f, sb = 0.f;
        for (int row = r0; row < r1; ++row) {
            const long o = (long)row * feat + c;
            const float g = dy[o];
            sg += g * (((x[o] + r[o]) - mean[row]) * rstd[row]);
            sb += g;
        }
        partial[((long)blockIdx.x * 2) * feat + c] = sg;
        partial[((long)blockIdx.x * 2 + 1) * feat + c] = sb;
    }
}

__global__ void __launch_bounds__(256)
ln_colreduce_kernel(const float* __restrict__ partial, int blocks, int feat, float* __restrict__ grad_gamma,
                    float* __restrict__ grad_beta) {
    I3D_CHAIN_PRIO();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * feat) return;
    const int which = t / feat, c = t - which * feat;
    float s = 0.f;
    for (int b = 0; b < blocks; ++b) s += partial[((long)b * 2 + which) * feat + c];
    (which ? grad_beta : grad_gamma)[c] = s;
}

// ---- pair head, pairs in destination-sorted (epos) order of the pair graph ------------------------------------------
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// out[perm[e], c] = softplus(u[i, c] + u[j, c] + 2 b[c]),  (i, j) = (src_s[e], dst_s[e])
__global__ void __launch_bounds__(256)
pair_sum_fwd_kernel(const float* __restrict__ u, const float* __restrict__ bias, const int* __restrict__ src_s,
                    const int* __restrict__ dst_s, const int* __restrict__ perm, int pairs, int feat, float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)pairs * feat) return;
    const int e = (int)(t / feat), c = (int)(t - (long)e * feat);
    const float x = (u[(long)src_s[e] * feat + c] + u[(long)dst_s[e] * feat + c]) + 2.f * bias[c];
    out[(long)perm[e] * feat + c] = softplus_f(x);
}

// grad_pair[e, c] = grad_out[perm[e], c] * sigmoid(u[i, c] + u[j, c] + 2 b[c])
__global__ void __launch_bounds__(256)
pair_sum_bwd_kernel(const float* __restrict__ grad_out, const float* __restrict__ u, const float* __restrict__ bias,
                    const int* __restrict__ src_s, const int* __restrict__ dst_s, const int* __restrict__ perm, int pairs,
                    int feat, float* __restrict__ grad_pair) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)pairs * feat) return;
    const int e = (int)(t / feat), c = (int)(t - (long)e * feat);
    const float x = (u[(long)src_s[e] * feat + c] + u[(long)dst_s[e] * feat + c]) + 2.f * bias[c];
    const float sg = x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
    grad_pair[t] = grad_out[(long)perm[e] * feat + c] * sg;
}

// out[perm[e]] = || p[i] - p[j] ||_2
__global__ void __launch_bounds__(256)
pair_norm_fwd_kernel(const float* __restrict__ p, const int* __restrict__ src_s, const int* __restrict__ dst_s,
                     const int* __restrict__ perm, int pairs, int feat, float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= pairs) return;
    const float* a = p + (long)src_s[e] * feat;
    const float* b = p + (long)dst_s[e] * feat;
    float s = 0.f;
    for (int c = 0; c < feat; ++c) {
        const float d = a[c] - b[c];
        s += d * d;
    }
    out[perm[e]] = sqrtf(s);
}

// grad_pair[e, 0:feat] = g (p[i] - p[j]) / d, grad_pair[e, feat:2 feat] = its negation (the destination's share);
// 0 at d = 0 (torch's subgradient of the norm there)
__global__ void __launch_bounds__(256)
pair_norm_bwd_kernel(const float* __restrict__ grad_out, const float* __restrict__ p, const float* __restrict__ dist,
                     const int* __restrict__ src_s, const int* __restrict__ dst_s, const int* __restrict__ perm, int pairs,
                     int feat, float* __restrict__ grad_pair) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)pairs * feat) return;
    const int e = (int)(t / feat), c = (int)(t - (long)e * feat);
    const int pid = perm[e];
    const float d = dist[pid];
    const float v = d > 0.f ? grad_out[pid] * (p[(long)src_s[e] * feat + c] - p[(long)dst_s[e] * feat + c]) / d : 0.f;
    grad_pair[(long)e * 2 * feat + c] = v;
    grad_pair[(long)e * 2 * feat + feat + c] = -v;
}

}  // namespace i3d

using namespace i3d;

static int mha_check(int num_graphs, int num_nodes, int hidden, int nhead) {
    I3D_CHECK_ARG(num_graphs >= 0 && num_nodes >= 0, "negative size");
    I3D_CHECK_ARG(hidden > 0 && nhead > 0 && hidden % nhead == 0, "hidden must be a positive multiple of nhead");
    I3D_CHECK_ARG(hidden / nhead <= ATT_MAX_DH, "head width hidden / nhead above 128");
    return I3D_OK;
}

extern "C" int i3d_mha_fwd(const float* qkv, const int* graph_ptr, int num_graphs, int num_nodes, int hidden, int nhead,
                           float scale, float* out, float* lse, void* stream) {
    if (int rc = mha_check(num_graphs, num_nodes, hidden, nhead)) return rc;
    I3D_CHECK_ARG(qkv && graph_ptr && out && lse, "null pointer");
    if (num_graphs == 0 || num_nodes == 0) return I3D_OK;
    const int dh = hidden / nhead;
    const size_t lds = sizeof(float) * (ATT_KT * (dh + 1) + ATT_KT * dh + ATT_WAVES * dh);
    const dim3 grid(num_graphs, nhead);
    if (dh <= 64)
        hipLaunchKernelGGL(mha_fwd_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, qkv, graph_ptr, hidden, nhead, dh,
                           scale, out, lse);
    else
        hipLaunchKernelGGL(mha_fwd_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, qkv, graph_ptr, hidden, nhead, dh,
                           scale, out, lse);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_mha_bwd(const float* qkv, const float* out, const float* grad_out, const float* lse, const int* graph_ptr,
                           int num_graphs, int num_nodes, int hidden, int nhead, float scale, float* delta, float* grad_qkv,
                           void* stream) {
    if (int rc = mha_check(num_graphs, num_nodes, hidden, nhead)) return rc;
    I3D_CHECK_ARG(qkv && out && grad_out && lse && graph_ptr && delta && grad_qkv, "null pointer");
    if (num_graphs == 0 || num_nodes == 0) return I3D_OK;
    const int dh = hidden / nhead;
    const size_t lds1 = sizeof(float) * (2 * ATT_KT * (dh + 1) + 2 * ATT_WAVES * dh);
    const size_t lds2 = lds1 + sizeof(float) * 2 * ATT_KT;
    const dim3 grid(num_graphs, nhead);
    hipStream_t s = (hipStream_t)stream;
    if (dh <= 64) {
        hipLaunchKernelGGL(mha_bwd_dq_kernel<1>, grid, dim3(256), lds1, s, qkv, out, grad_out, lse, graph_ptr, hidden, nhead, dh,
                           scale, delta, grad_qkv);
        hipLaunchKernelGGL(mha_bwd_dkv_kernel<1>, grid, dim3(256), lds2, s, qkv, grad_out, lse, delta, graph_ptr, hidden, nhead,
                           dh, scale, grad_qkv);
    } else {
        hipLaunchKernelGGL(mha_bwd_dq_kernel<2>, grid, dim3(256), lds1, s, qkv, out, grad_out, lse, graph_ptr, hidden, nhead, dh,
                           scale, delta, grad_qkv);
        hipLaunchKernelGGL(mha_bwd_dkv_kernel<2>, grid, dim3(256), lds2, s, qkv, grad_out, lse, delta, graph_ptr, hidden, nhead,
                           dh, scale, grad_qkv);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_ln_res_fwd(const float* x, const float* r, const float* gamma, const float* beta, int rows, int feat,
                              float eps, float* y, float* mean, float* rstd, void* stream) {
    I3D_CHECK_ARG(rows >= 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(x && r && gamma && beta && y && mean && rstd, "null pointer");
    if (rows == 0) return I3D_OK;
    hipLaunchKernelGGL(ln_res_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, r, gamma, beta, rows, feat,
                       eps, y, mean, rstd);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" long i3d_ln_res_partial_floats(int rows, int feat) { return 2L * cdiv(rows > 0 ? rows : 1, LN_ROWS) * feat; }

extern "C" int i3d_ln_res_bwd(const float* grad_y, const float* x, const float* r, const float* gamma, const float* mean,
                              const float* rstd, int rows, int feat, float* grad_x, float* partial, float* grad_gamma,
                              float* grad_beta, void* stream) {
    I3D_CHECK_ARG(rows > 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(grad_y && x && r && gamma && mean && rstd && grad_x && partial && grad_gamma && grad_beta, "null pointer");
    const int blocks = cdiv(rows, LN_ROWS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ln_res_bwd_kernel, dim3(blocks), dim3(256), 0, s, grad_y, x, r, gamma, mean, rstd, rows, feat, grad_x,
                       partial);
    hipLaunchKernelGGL(ln_colreduce_kernel, dim3(cdiv(2L * feat, 256)), dim3(256), 0, s, partial, blocks, feat, grad_gamma,
                       grad_beta);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_pair_sum_fwd(const float* u, const float* bias, const int* src_s, const int* dst_s, const int* perm,
                                int pairs, int feat, float* out, void* stream) {
    I3D_CHECK_ARG(pairs >= 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(u && bias && src_s && dst_s && perm && out, "null pointer");
    if (pairs == 0) return I3D_OK;
    hipLaunchKernelGGL(pair_sum_fwd_kernel, dim3(cdiv((long)pairs * feat, 256)), dim3(256), 0, (hipStream_t)stream, u, bias,
                       src_s, dst_s, perm, pairs, feat, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_pair_sum_bwd(const float* grad_out, const float* u, const float* bias, const int* src_s, const int* dst_s,
                                const int* perm, int pairs, int feat, float* grad_pair, void* stream) {
    I3D_CHECK_ARG(pairs >= 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(grad_out && u && bias && src_s && dst_s && perm && grad_pair, "null pointer");
    if (pairs == 0) return I3D_OK;
    hipLaunchKernelGGL(pair_sum_bwd_kernel, dim3(cdiv((long)pairs * feat, 256)), dim3(256), 0, (hipStream_t)stream, grad_out, u,
                       bias, src_s, dst_s, perm, pairs, feat, grad_pair);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_pair_norm_fwd(const float* p, const int* src_s, const int* dst_s, const int* perm, int pairs, int feat,
                                 float* out, void* stream) {
    I3D_CHECK_ARG(pairs >= 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(p && src_s && dst_s && perm && out, "null pointer");
    if (pairs == 0) return I3D_OK;
    hipLaunchKernelGGL(pair_norm_fwd_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, (hipStream_t)stream, p, src_s, dst_s, perm,
                       pairs, feat, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_pair_norm_bwd(const float* grad_out, const float* p, const float* dist, const int* src_s, const int* dst_s,
                                 const int* perm, int pairs, int feat, float* grad_pair, void* stream) {
    I3D_CHECK_ARG(pairs >= 0 && feat > 0, "bad shape");
    I3D_CHECK_ARG(grad_out && p && dist && src_s && dst_s && perm && grad_pair, "null pointer");
    if (pairs == 0) return I3D_OK;
    hipLaunchKernelGGL(pair_norm_bwd_kernel, dim3(cdiv((long)pairs * feat, 256)), dim3(256), 0, (hipStream_t)stream, grad_out,
                       p, dist, src_s, dst_s, perm, pairs, feat, grad_pair);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
