// SAN's edge attention (reference models/san.py:111-177, MultiHeadAttentionLayer.propagate_attention and the division by the
// normaliser), both directions, with the two edge projections E(e), E_2(e) as rows of two [V, H] tables of all bond-feature
// combinations.  Per head a of width dh = H / nh, for an edge j -> i at position p (destination-sorted) with code c_p and flag real_p:
//
//   s_p[a]   = (1 / sqrt(dh)) sum_{d in head a} Ksel_j[d] Qsel_i[d] Tsel[c_p][d]     (K, Q, TE) real or not full_graph, else (K_2, Q_2, TE2)
//   w_p[a]   = exp(clamp(s_p[a], -5, 5)) coef          coef = 1 / (gamma + 1) real, gamma / (gamma + 1) fake, 1 if not full_graph
//   out_i[d] = sum_p w_p[a] V_j[d] / (sum_p w_p[a] + 1e-6)
//
// No [E, H] tensor exists in either direction.  The forward keeps s [E, nh] and the normaliser z [N, nh]; the backward recomputes w
// and the clamp gate (s inside [-5, 5], torch's clamp backward) from s and passes ds [E, nh] from its destination pass to its source
// and table passes.
//
// Lane map.  One wave owns a node.  A head takes a group of G lanes, G the power of two with G >= max(dh, 4), one column per lane
// (lanes >= dh of a group idle); the wave has S = 64 / G groups.  nh >= S: the heads go through R = ceil(nh / S) passes, one edge per
// wave-instruction.  nh < S: R = 1 and the wave takes S / nh consecutive edges at once, edge slot `sub` on lanes [sub nh G, (sub + 1) nh G).
// A head's sum is an xor-butterfly inside its group; the per-slot running sums are added in slot order after the last edge.  Every
// sum has a fixed order: no atomics, the same bits on every call.
//
// i3d_san_edge_codes gives the kernels their per-edge inputs in one launch: the joint bond code and the uint8 real flag of every
// edge position, 5 bytes per edge (i3d_edge_codes also writes a one-hot row per edge, as wide as an [E, H] row at H = 64).
//
// Limits (anything else is I3D_NOT_TAKEN, the caller composes the step): H % nh == 0 (else invalid), dh <= 64,
// ceil(nh / (64 / G)) <= 8 - nh G <= 512, e.g. H <= 512 at dh = 64, nh <= 16 at dh <= 32, nh <= 128 at dh <= 4 -, V <= 256.
//
//   forward         wave = destination i: Q_i, Q2_i in registers; per in-edge K / V / table rows gathered, SAN_U(R) edges in flight.
//   backward 1      wave = destination i: gn_i = g_i / (z_i + 1e-6) (written, [N, H]); per in-edge dw = <gn_i, V_j - out_i> over the
//                   head, ds = dw w gate / sqrt(dh) (written, [E, nh]); dQ_i, dQ2_i = sum ds K_j T.
//   backward 2      wave = source j over its out-edges (out_ptr / out_epos order): dV_j = sum w gn_i, dK_j, dK2_j = sum ds Q_i T.
//   backward 3, 4   dTE, dTE2 as csrc/gin.hip reduces its table gradient: fp64 over FIXED chunks of SAN_CHUNK positions of the
//                   code-sorted edge list (a run is closed whenever the code changes; run (k, c) goes to slot k + c), then per code
//                   over its chunks - four waves, each a quarter of the chunks in chunk order, the four sums in wave order -,
//                   rounded once.  Nearly all fake edges share code 0: its second stage adds one partial per chunk, not one
//                   term per edge, and not in one thread's chain.  A code without edges gets a zero row.
#include "common.h"

namespace i3d {

constexpr int SAN_CHUNK = 128;            // positions of the code-sorted list per table-gradient workgroup
constexpr int SAN_MAX_CODES = 256;
constexpr int SAN_FINAL_PARTS = 4;      // waves of a table-gradient final workgroup, each with a quarter of the code's chunks
constexpr int SAN_MAX_HEAD = 64;          // dh
constexpr int SAN_MAX_PASSES = 8;         // R
constexpr float SAN_CLAMP = 5.f;
constexpr float SAN_EPS = 1e-6f;

constexpr int san_unroll(int R) { return R >= 4 ? 2 : 4; }      // edges in flight per wave: R passes x 3-5 loads each

// sum over the G lanes of a head's group: every lane of the group gets it
template <int G>
__device__ __forceinline__ float san_group_sum(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <int G, int R>
struct SanLane {
    int l, sub, epw, stride, passes;      // lane in its group, edge slot, edge slots of the wave, lanes between two slots, live passes
    int head[R], col[R];
    bool live[R];
    __device__ __forceinline__ SanLane(int lane, int nh, int dh) {
        constexpr int S = WAVE / G;
        const int slot = lane / G;
        l = lane % G;
        epw = nh < S ? S / nh : 1;
        stride = nh * G;
        sub = nh < S ? slot / nh : 0;
        passes = (nh + S - 1) / S;            // R is rounded up to 1, 2, 4, 8: the passes beyond this hold no head
#pragma unroll
        for (int r = 0; r < R; ++r) {
            head[r] = nh < S ? slot % nh : r * S + slot;
            live[r] = head[r] < nh && l < dh && sub < epw;
            col[r] = head[r] * dh + l;
        }
    }
    // the slots' sums in slot order; the lanes of slot 0 hold the result
    __device__ __forceinline__ float slot_sum(float v, int lane) const {
        float s = v;
        for (int k = 1; k < epw; ++k) s += __shfl(v, (lane + k * stride) & (WAVE - 1));
        return s;
    }
};

__device__ __forceinline__ float san_weight(float s, float coef) {
    return expf(fminf(fmaxf(s, -SAN_CLAMP), SAN_CLAMP)) * coef;
}

template <int G, int R>
__global__ void __launch_bounds__(256)
san_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const float* __restrict__ q2,
                    const float* __restrict__ k2, int ld, const float* __restrict__ te, const float* __restrict__ te2,
                    const int* __restrict__ codes, const unsigned char* __restrict__ real, const int* __restrict__ in_ptr,
                    const int* __restrict__ src_s, int N, int H, int nh, int dh, float scale, float coef_real, float coef_fake,
                    float* __restrict__ out, float* __restrict__ s_out, float* __restrict__ z_out) {
    I3D_CHAIN_PRIO();
    constexpr int U = san_unroll(R);
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                            // whole waves
    const int lane = threadIdx.x & 63;
    const SanLane<G, R> m(lane, nh, dh);
    float qv[R], q2v[R], acc[R], zacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        qv[r] = m.live[r] ? q[(long)i * ld + m.col[r]] : 0.f;
        q2v[r] = (m.live[r] && q2) ? q2[(long)i * ld + m.col[r]] : 0.f;
        acc[r] = zacc[r] = 0.f;
    }
    const int beg = in_ptr[i], end = in_ptr[i + 1];
    for (int j0 = beg; j0 < end; j0 += U * m.epw) {
        float kk[U][R], vv[U][R], tt[U][R];
        bool rl[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int e = j0 + t * m.epw + m.sub;
            const bool ok = e < end && m.sub < m.epw;
            int src = 0, code = 0;
            rl[t] = true;
            if (ok) {
                src = src_s[e];
                code = codes[e];
                if (real) rl[t] = real[e] != 0;
            }
            const float* kp = rl[t] ? k : k2;
            const float* tp = rl[t] ? te : te2;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool on = ok && m.live[r];
                kk[t][r] = on ? kp[(long)src * ld + m.col[r]] : 0.f;
                vv[t][r] = on ? v[(long)src * ld + m.col[r]] : 0.f;
                tt[t][r] = on ? tp[(long)code * H + m.col[r]] : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int e = j0 + t * m.epw + m.sub;
            const bool ok = e < end && m.sub < m.epw;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= m.passes) continue;       // wave-uniform
                const float s = san_group_sum<G>(kk[t][r] * (rl[t] ? qv[r] : q2v[r]) * tt[t][r]) * scale;
                const float w = san_weight(s, rl[t] ? coef_real : coef_fake);
                if (ok && m.live[r]) {
                    acc[r] += w * vv[t][r];
                    zacc[r] += w;
                    if (m.l == 0) s_out[(long)e * nh + m.head[r]] = s;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float a = m.slot_sum(acc[r], lane), z = m.slot_sum(zacc[r], lane);
        if (m.sub == 0 && m.live[r]) {
            out[(long)i * H + m.col[r]] = a / (z + SAN_EPS);       // no in-edges: 0 / 1e-6, an exact zero row
            if (m.l == 0) z_out[(long)i * nh + m.head[r]] = z;
        }
    }
}

template <int G, int R>
__global__ void __launch_bounds__(256)
san_attn_bwd_dst_kernel(const float* __restrict__ g, const float* __restrict__ out, const float* __restrict__ z,
                        const float* __restrict__ s_saved, const float* __restrict__ q, const float* __restrict__ k,
                        const float* __restrict__ v, const float* __restrict__ q2, const float* __restrict__ k2, int ld,
                        const float* __restrict__ te, const float* __restrict__ te2, const int* __restrict__ codes,
                        const unsigned char* __restrict__ real, const int* __restrict__ in_ptr, const int* __restrict__ src_s, int N,
                        int H, int nh, int dh, float scale, float coef_real, float coef_fake, float* __restrict__ gn,
                        float* __restrict__ ds, float* __restrict__ dq, float* __restrict__ dq2, int ldg) {
    I3D_CHAIN_PRIO();
    constexpr int U = san_unroll(R);
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int lane = threadIdx.x & 63;
    const SanLane<G, R> m(lane, nh, dh);
    float gnv[R], ov[R], aq[R], aq2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        gnv[r] = ov[r] = aq[r] = aq2[r] = 0.f;
        if (m.live[r]) {
            gnv[r] = g[(long)i * H + m.col[r]] / (z[(long)i * nh + m.head[r]] + SAN_EPS);
            ov[r] = out[(long)i * H + m.col[r]];
            if (m.sub == 0) gn[(long)i * H + m.col[r]] = gnv[r];
        }
    }
    const int beg = in_ptr[i], end = in_ptr[i + 1];
    for (int j0 = beg; j0 < end; j0 += U * m.epw) {
        float kk[U][R], vv[U][R], tt[U][R], sv[U][R];
        bool rl[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int e = j0 + t * m.epw + m.sub;
            const bool ok = e < end && m.sub < m.epw;
            int src = 0, code = 0;
            rl[t] = true;
            if (ok) {
                src = src_s[e];
                code = codes[e];
                if (real) rl[t] = real[e] != 0;
            }
            const float* kp = rl[t] ? k : k2;
            const float* tp = rl[t] ? te : te2;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool on = ok && m.live[r];
                kk[t][r] = on ? kp[(long)src * ld + m.col[r]] : 0.f;
                vv[t][r] = on ? v[(long)src * ld + m.col[r]] : 0.f;
                tt[t][r] = on ? tp[(long)code * H + m.col[r]] : 0.f;
                sv[t][r] = on ? s_saved[(long)e * nh + m.head[r]] : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int e = j0 + t * m.epw + m.sub;
            const bool ok = e < end && m.sub < m.epw;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= m.passes) continue;       // wave-uniform
                const float dw = san_group_sum<G>(gnv[r] * (vv[t][r] - ov[r]));
                const float s = sv[t][r];
                const bool gate = s >= -SAN_CLAMP && s <= SAN_CLAMP;
                const float d = gate ? dw * san_weight(s, rl[t] ? coef_real : coef_fake) * scale : 0.f;
                if (ok && m.live[r]) {
                    if (m.l == 0) ds[(long)e * nh + m.head[r]] = d;
                    const float kt = d * kk[t][r] * tt[t][r];
                    if (rl[t]) aq[r] += kt; else aq2[r] += kt;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float a = m.slot_sum(aq[r], lane), a2 = m.slot_sum(aq2[r], lane);
        if (m.sub == 0 && m.live[r]) {
            dq[(long)i * ldg + m.col[r]] = a;
            if (dq2) dq2[(long)i * ldg + m.col[r]] = a2;
        }
    }
}

template <int G, int R>
__global__ void __launch_bounds__(256)
san_attn_bwd_src_kernel(const float* __restrict__ gn, const float* __restrict__ s_saved, const float* __restrict__ ds,
                        const float* __restrict__ q, const float* __restrict__ q2, int ld, const float* __restrict__ te,
                        const float* __restrict__ te2, const int* __restrict__ codes, const unsigned char* __restrict__ real,
                        const int* __restrict__ dst_s, const int* __restrict__ out_ptr, const int* __restrict__ out_epos, int N, int H,
                        int nh, int dh, float coef_real, float coef_fake, float* __restrict__ dk, float* __restrict__ dv,
                        float* __restrict__ dk2, int ldg) {
    I3D_CHAIN_PRIO();
    constexpr int U = san_unroll(R);
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    const int lane = threadIdx.x & 63;
    const SanLane<G, R> m(lane, nh, dh);
    float ak[R], ak2[R], av[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ak[r] = ak2[r] = av[r] = 0.f;
    const int beg = out_ptr[j], end = out_ptr[j + 1];
    for (int p0 = beg; p0 < end; p0 += U * m.epw) {
        float gg[U][R], qq[U][R], tt[U][R], sv[U][R], dd[U][R];
        bool rl[U];
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int p = p0 + t * m.epw + m.sub;
            const bool ok = p < end && m.sub < m.epw;
            int e = 0, dst = 0, code = 0;
            rl[t] = true;
            if (ok) {
                e = out_epos[p];
                dst = dst_s[e];
                code = codes[e];
                if (real) rl[t] = real[e] != 0;
            }
            const float* qp = rl[t] ? q : q2;
            const float* tp = rl[t] ? te : te2;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool on = ok && m.live[r];
                gg[t][r] = on ? gn[(long)dst * H + m.col[r]] : 0.f;
                qq[t][r] = on ? qp[(long)dst * ld + m.col[r]] : 0.f;
                tt[t][r] = on ? tp[(long)code * H + m.col[r]] : 0.f;
                sv[t][r] = on ? s_saved[(long)e * nh + m.head[r]] : 0.f;
                dd[t][r] = on ? ds[(long)e * nh + m.head[r]] : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
            const int p = p0 + t * m.epw + m.sub;
            const bool ok = p < end && m.sub < m.epw;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (ok && m.live[r]) {
                    av[r] += san_weight(sv[t][r], rl[t] ? coef_real : coef_fake) * gg[t][r];
                    const float kt = dd[t][r] * qq[t][r] * tt[t][r];
                    if (rl[t]) ak[r] += kt; else ak2[r] += kt;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float a = m.slot_sum(ak[r], lane), a2 = m.slot_sum(ak2[r], lane), b = m.slot_sum(av[r], lane);
        if (m.sub == 0 && m.live[r]) {
            dk[(long)j * ldg + m.col[r]] = a;
            dv[(long)j * ldg + m.col[r]] = b;
            if (dk2) dk2[(long)j * ldg + m.col[r]] = a2;
        }
    }
}

// workgroup (k, column tile): positions [k SAN_CHUNK, (k + 1) SAN_CHUNK) of the code-sorted list, thread = one column, the block as
// wide as the row up to 256 threads (H = 64: one wave, none idle); the real
// edges' runs go to plane 0 of the partials (dTE), the fake edges' to plane 1 (dTE2)
__global__ void __launch_bounds__(256)
san_attn_bwd_table_chunk_kernel(const float* __restrict__ ds, const float* __restrict__ q, const float* __restrict__ k,
                                const float* __restrict__ q2, const float* __restrict__ k2, int ld, const int* __restrict__ codes,
                                const unsigned char* __restrict__ real, const int* __restrict__ src_s, const int* __restrict__ dst_s,
                                const int* __restrict__ order, int E, int H, int nh, int dh, long plane, double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ int s_e[SAN_CHUNK], s_src[SAN_CHUNK], s_dst[SAN_CHUNK], s_code[SAN_CHUNK], s_real[SAN_CHUNK];
    const int p0 = blockIdx.x * SAN_CHUNK, n = min(SAN_CHUNK, E - p0);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int e = order[p0 + i];
        s_e[i] = e;
        s_src[i] = src_s[e];
        s_dst[i] = dst_s[e];
        s_code[i] = codes[e];
        s_real[i] = real ? (real[e] != 0) : 1;
    }
    __syncthreads();
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= H) return;
    const int head = c / dh;
    int code = s_code[0];
    double acc = 0., acc2 = 0.;
    for (int i = 0; i < n; ++i) {
        const int ci = s_code[i];
        if (ci != code) {
            partial[((long)blockIdx.x + code) * H + c] = acc;
            partial[plane + ((long)blockIdx.x + code) * H + c] = acc2;
            code = ci;
            acc = acc2 = 0.;
        }
        const double d = (double)ds[(long)s_e[i] * nh + head];
        if (s_real[i]) acc += d * (double)k[(long)s_src[i] * ld + c] * (double)q[(long)s_dst[i] * ld + c];
        else acc2 += d * (double)k2[(long)s_src[i] * ld + c] * (double)q2[(long)s_dst[i] * ld + c];
    }
    partial[((long)blockIdx.x + code) * H + c] = acc;
    partial[plane + ((long)blockIdx.x + code) * H + c] = acc2;
}

// workgroup = (one code, 64 columns): its rows of dTE and dTE2 from the partials of its chunks.  Code 0 holds nearly all fake edges,
// so its chunks are many (E / 128): wave w adds the w-th quarter of them in chunk order, the loads of a quarter issued eight at a
// time, and the four sums are added in wave order
__global__ void __launch_bounds__(256)
san_attn_bwd_table_final_kernel(const double* __restrict__ partial, long plane, const int* __restrict__ code_ptr, int H,
                                float* __restrict__ dte, float* __restrict__ dte2) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[2][SAN_FINAL_PARTS][WAVE];
    const int code = blockIdx.x, lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.y * WAVE + lane;
    const int a = code_ptr[code], b = code_ptr[code + 1];
    double s = 0., s2 = 0.;
    if (b > a && c < H) {
        const int k0 = a / SAN_CHUNK, k1 = (b - 1) / SAN_CHUNK;
        const int per = (k1 - k0 + SAN_FINAL_PARTS) / SAN_FINAL_PARTS;
        const int lo = k0 + part * per, hi = min(lo + per, k1 + 1);
#pragma unroll 8
        for (int k = lo; k < hi; ++k) {
            s += partial[((long)k + code) * H + c];
            if (dte2) s2 += partial[plane + ((long)k + code) * H + c];
        }
    }
    sm[0][part][lane] = s;
    sm[1][part][lane] = s2;
    __syncthreads();
    if (part == 0 && c < H) {
        dte[(long)code * H + c] = (float)(((sm[0][0][lane] + sm[0][1][lane]) + sm[0][2][lane]) + sm[0][3][lane]);
        if (dte2) dte2[(long)code * H + c] = (float)(((sm[1][0][lane] + sm[1][1][lane]) + sm[1][2][lane]) + sm[1][3][lane]);
    }
}

struct SanStrides {
    int s[8];
};

// thread = edge position p: the joint code of row perm[p] of the bond features and its real flag, nothing else written
__global__ void __launch_bounds__(256)
san_edge_codes_kernel(const long* __restrict__ feat, const long* __restrict__ real_in, const int* __restrict__ perm, int E, int n_cols,
                      SanStrides st, int* __restrict__ codes, unsigned char* __restrict__ real) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= E) return;
    const long row = perm[p];
    int code = 0;
    for (int c = 0; c < n_cols; ++c) code += (int)feat[row * n_cols + c] * st.s[c];
    codes[p] = code;
    if (real) real[p] = real_in[row] != 0;
}

struct SanPlan {
    int dh, G, R;
};

// I3D_OK with the plan filled in, I3D_NOT_TAKEN outside the lane map, I3D_ERR_INVALID on impossible sizes
static int san_plan(const char* who, int num_nodes, int num_edges, int feat, int heads, int num_codes, SanPlan* p) {
    if (num_nodes < 0 || num_edges < 0 || feat < 1 || heads < 1 || num_codes < 1 || feat % heads != 0) {
        set_error("%s: invalid argument: num_nodes / num_edges below 0, feat / heads / num_codes below 1 or feat %% heads != 0", who);
        return I3D_ERR_INVALID;
    }
    p->dh = feat / heads;
    if (p->dh > SAN_MAX_HEAD || num_codes > SAN_MAX_CODES) return I3D_NOT_TAKEN;
    p->G = 4;
    while (p->G < p->dh) p->G <<= 1;
    const int S = WAVE / p->G, passes = (heads + S - 1) / S;
    if (passes > SAN_MAX_PASSES) return I3D_NOT_TAKEN;
    p->R = passes <= 1 ? 1 : (passes <= 2 ? 2 : (passes <= 4 ? 4 : 8));
    return I3D_OK;
}

}  // namespace i3d

using namespace i3d;

#define SAN_DISPATCH_R(KERNEL, GG, ...)                                                                                            \
    do {                                                                                                                           \
        if (plan.R == 1) hipLaunchKernelGGL((KERNEL<GG, 1>), grid_, dim3(256), 0, s_, __VA_ARGS__);                                \
        else if (plan.R == 2) hipLaunchKernelGGL((KERNEL<GG, 2>), grid_, dim3(256), 0, s_, __VA_ARGS__);                           \
        else if (plan.R == 4) hipLaunchKernelGGL((KERNEL<GG, 4>), grid_, dim3(256), 0, s_, __VA_ARGS__);                           \
        else hipLaunchKernelGGL((KERNEL<GG, 8>), grid_, dim3(256), 0, s_, __VA_ARGS__);                                            \
    } while (0)

#define SAN_DISPATCH(KERNEL, ...)                                                                                                  \
    do {                                                                                                                           \
        const dim3 grid_(cdiv(num_nodes, 4));                                                                                      \
        hipStream_t s_ = (hipStream_t)stream;                                                                                      \
        if (plan.G == 4) SAN_DISPATCH_R(KERNEL, 4, __VA_ARGS__);                                                                   \
        else if (plan.G == 8) SAN_DISPATCH_R(KERNEL, 8, __VA_ARGS__);                                                              \
        else if (plan.G == 16) SAN_DISPATCH_R(KERNEL, 16, __VA_ARGS__);                                                            \
        else if (plan.G == 32) SAN_DISPATCH_R(KERNEL, 32, __VA_ARGS__);                                                            \
        else SAN_DISPATCH_R(KERNEL, 64, __VA_ARGS__);                                                                              \
    } while (0)

extern "C" int i3d_san_attn_chunk_edges(void) { return SAN_CHUNK; }

extern "C" int i3d_san_edge_codes(const int64_t* feat, const int64_t* real_in, const int* perm, int num_edges, int n_cols,
                                  const int* strides, int* codes, unsigned char* real, void* stream) {
    I3D_CHECK_ARG(num_edges >= 0 && n_cols >= 1 && n_cols <= 8, "num_edges below 0 or n_cols outside 1..8");
    I3D_CHECK_ARG(strides, "null pointer");
    if (num_edges == 0) return I3D_OK;
    I3D_CHECK_ARG(feat && perm && codes && (!real == !real_in), "null pointer, or one of real_in / real without the other");
    SanStrides st;
    for (int c = 0; c < 8; ++c) st.s[c] = c < n_cols ? strides[c] : 0;
    hipLaunchKernelGGL(san_edge_codes_kernel, dim3(cdiv(num_edges, 256)), dim3(256), 0, (hipStream_t)stream, (const long*)feat,
                       (const long*)real_in, perm, num_edges, n_cols, st, codes, real);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_san_attn_takes(int feat, int heads, int num_codes) {
    SanPlan plan;
    return san_plan("i3d_san_attn_takes", 1, 0, feat, heads, num_codes, &plan);
}

extern "C" long i3d_san_attn_bwd_partial_floats(int num_edges, int feat, int num_codes) {
    if (num_edges < 0 || feat < 1 || num_codes < 1 || num_codes > SAN_MAX_CODES) return 0;
    const long chunks = ((long)num_edges + SAN_CHUNK - 1) / SAN_CHUNK;
    return 2L * 2L * (chunks + num_codes) * feat;        // two planes of fp64
}

extern "C" int i3d_san_attn_fwd(const float* q, const float* k, const float* v, const float* q2, const float* k2, int ld,
                                const float* te, const float* te2, int num_codes, const int* codes, const unsigned char* real,
                                const int* in_ptr, const int* src_s, int num_nodes, int num_edges, int feat, int heads, int full_graph,
                                float gamma, float* out, float* s, float* z, void* stream) {
    SanPlan plan;
    if (int rc = san_plan(__func__, num_nodes, num_edges, feat, heads, num_codes, &plan)) return rc;
    I3D_CHECK_ARG(ld >= feat, "ld below feat");
    I3D_CHECK_ARG(q && k && v && te && in_ptr && out && z, "null pointer");
    I3D_CHECK_ARG(!full_graph || (q2 && k2 && te2), "full_graph without q2 / k2 / te2");
    I3D_CHECK_ARG(num_edges == 0 || (codes && src_s && s && (!full_graph || real)), "edges without codes / src_s / s / real");
    if (num_nodes == 0) return I3D_OK;
    const float scale = 1.f / sqrtf((float)plan.dh);
    const float coef_real = full_graph ? 1.f / (gamma + 1.f) : 1.f, coef_fake = full_graph ? gamma / (gamma + 1.f) : 1.f;
    if (!full_graph) q2 = k2 = te2 = nullptr, real = nullptr;
    SAN_DISPATCH(san_attn_fwd_kernel, q, k, v, q2, k2, ld, te, te2, codes, real, in_ptr, src_s, num_nodes, feat, heads, plan.dh, scale,
                 coef_real, coef_fake, out, s, z);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_san_attn_bwd(const float* g, const float* out, const float* z, const float* s, const float* q, const float* k,
                                const float* v, const float* q2, const float* k2, int ld, const float* te, const float* te2,
                                int num_codes, const int* codes, const unsigned char* real, const int* in_ptr, const int* src_s,
                                const int* dst_s, const int* out_ptr, const int* out_epos, const int* code_order, const int* code_ptr,
                                int num_nodes, int num_edges, int feat, int heads, int full_graph, float gamma, float* gn, float* ds,
                                float* partials, float* dq, float* dk, float* dv, float* dq2, float* dk2, int ldg, float* dte,
                                float* dte2, void* stream) {
    SanPlan plan;
    if (int rc = san_plan(__func__, num_nodes, num_edges, feat, heads, num_codes, &plan)) return rc;
    I3D_CHECK_ARG(ld >= feat && ldg >= feat, "ld / ldg below feat");
    I3D_CHECK_ARG(g && out && z && q && k && v && te && in_ptr && out_ptr && code_ptr && gn && partials && dq && dk && dv && dte,
                  "null pointer");
    I3D_CHECK_ARG(!full_graph || (q2 && k2 && te2 && dq2 && dk2 && dte2), "full_graph without the second set's tensors");
    I3D_CHECK_ARG(num_edges == 0 || (s && ds && codes && src_s && dst_s && out_epos && code_order && (!full_graph || real)),
                  "edges without their index arrays / s / ds / real");
    I3D_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "partials not 8-byte aligned");
    if (num_nodes == 0) return I3D_OK;
    const float scale = 1.f / sqrtf((float)plan.dh);
    const float coef_real = full_graph ? 1.f / (gamma + 1.f) : 1.f, coef_fake = full_graph ? gamma / (gamma + 1.f) : 1.f;
    if (!full_graph) q2 = k2 = te2 = nullptr, real = nullptr, dq2 = dk2 = dte2 = nullptr;
    SAN_DISPATCH(san_attn_bwd_dst_kernel, g, out, z, s, q, k, v, q2, k2, ld, te, te2, codes, real, in_ptr, src_s, num_nodes, feat, heads,
                 plan.dh, scale, coef_real, coef_fake, gn, ds, dq, dq2, ldg);
    I3D_CHECK_LAUNCH();
    SAN_DISPATCH(san_attn_bwd_src_kernel, (const float*)gn, s, (const float*)ds, q, q2, ld, te, te2, codes, real, dst_s, out_ptr,
                 out_epos, num_nodes, feat, heads, plan.dh, coef_real, coef_fake, dk, dv, dk2, ldg);
    I3D_CHECK_LAUNCH();
    const int chunks = cdiv(num_edges, SAN_CHUNK);
    double* part = reinterpret_cast<double*>(partials);
    const long plane = ((long)chunks + num_codes) * feat;
    if (chunks > 0) {
        const int threads = feat >= 256 ? 256 : cdiv(feat, WAVE) * WAVE;
        hipLaunchKernelGGL(san_attn_bwd_table_chunk_kernel, dim3(chunks, cdiv(feat, threads)), dim3(threads), 0, (hipStream_t)stream,
                           (const float*)ds, q, k, q2, k2, ld, codes, real, src_s, dst_s, code_order, num_edges, feat, heads, plan.dh,
                           plane, part);
        I3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(san_attn_bwd_table_final_kernel, dim3(num_codes, cdiv(feat, WAVE)), dim3(256), 0, (hipStream_t)stream, (const double*)part, plane,
                       code_ptr, feat, dte, dte2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
