// EGNN's soft-edge gate, the reduction over the in-edges and the residual add in one launch per direction (reference
// models/egnn.py:124-137: message * sigmoid(soft_edge_network(message)), fn.sum / fn.mean, m_sum + feat):
//
//   w[j] = sigmoid(<ws, m[j]> + bs)                          j an edge, m [E, H] destination-sorted
//   u[v] = h[v] + red_{j in [in_ptr[v], in_ptr[v+1])} m[j] w[j]        red = sum, or sum / in-degree (a node without in-edges: u = h)
//
// Neither m * w nor its gradient exists as an [E, H] tensor: the forward reads m once and keeps the gate, 4 bytes per edge; the
// backward reads m once and writes dL/dm once.
//
// Layout.  One wave owns a destination.  A row of H floats is spread over G lanes (G the power of two with 4 G >= H, at least 8, at
// most 64), four consecutive columns per lane and load (16 bytes); with H above 256 a lane owns a second group of four, 256 columns
// further on.  The 64 / G lane groups of the wave take consecutive edges, so one wave-instruction loads 64 / G rows (two at H = 128),
// and GR_UNROLL such instructions are issued before the first dot product is reduced: 8 rows of 512 bytes in flight per wave at
// H = 128.  The dot product of an edge is reduced inside its lane group by xor-shuffles; the per-group running sums are added
// across the groups once, after the last edge, again by xor-shuffles.  Every sum has a fixed order: no atomics, the same bits on
// every call.
//
//   backward   g = dL/du[v] (divided by the in-degree for the mean), D_j = <g, m[j]>, gg_j = D_j w_j (1 - w_j),
//              dL/dm[j] = g w_j + gg_j ws.  The same wave adds up gg_j m[j] and gg_j over its edges and writes them as row v of
//              the partials [N, H] and [N]: the column sum over the nodes (i3d_colsum, fixed order) finishes dL/dws and dL/dbs.
//              dL/dh = dL/du is the caller's.
#include "common.h"

namespace i3d {

constexpr int GR_MAX_FEAT = 512;
constexpr int GR_UNROLL = 4;

__device__ __forceinline__ float4 gr_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float gr_dot(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// sum over the G lanes of a group (G a power of two): every lane of the group gets it
template <int G>
__device__ __forceinline__ float gr_group_sum(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the 64 / G groups of the wave, lane by lane
template <int G>
__device__ __forceinline__ float gr_cross_sum(float v) {
#pragma unroll
    for (int o = G; o < WAVE; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <int G>
__device__ __forceinline__ float4 gr_cross_sum4(float4 v) {
    return make_float4(gr_cross_sum<G>(v.x), gr_cross_sum<G>(v.y), gr_cross_sum<G>(v.z), gr_cross_sum<G>(v.w));
}

template <int G, int R>
__global__ void __launch_bounds__(256)
gate_reduce_fwd_kernel(const float* __restrict__ m, const float* __restrict__ ws, const float* __restrict__ bs,
                       const int* __restrict__ in_ptr, const float* __restrict__ h, int N, int H, int reduce_mean,
                       float* __restrict__ u, float* __restrict__ w) {
    I3D_CHAIN_PRIO();
    constexpr int S = WAVE / G;                    // edges per wave-instruction
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;                            // whole waves
    const int lane = threadIdx.x & 63, sub = lane / G, l = lane % G;
    int col[R];
    bool live[R];
    float4 wv[R], acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        col[k] = l * 4 + k * 256;
        live[k] = col[k] < H;
        wv[k] = live[k] ? *reinterpret_cast<const float4*>(ws + col[k]) : gr_zero();
        acc[k] = gr_zero();
    }
    const float bias = bs[0];
    const int beg = in_ptr[v], end = in_ptr[v + 1];
    for (int j0 = beg; j0 < end; j0 += GR_UNROLL * S) {
        float4 x[GR_UNROLL][R];
#pragma unroll
        for (int t = 0; t < GR_UNROLL; ++t) {
            const int e = j0 + t * S + sub;
#pragma unroll
            for (int k = 0; k < R; ++k)
                x[t][k] = (e < end && live[k]) ? *reinterpret_cast<const float4*>(m + (long)e * H + col[k]) : gr_zero();
        }
#pragma unroll
        for (int t = 0; t < GR_UNROLL; ++t) {
            const int e = j0 + t * S + sub;
            float dot = gr_dot(x[t][0], wv[0]);
#pragma unroll
            for (int k = 1; k < R; ++k) dot += gr_dot(x[t][k], wv[k]);
            dot = gr_group_sum<G>(dot);
            const float gate = 1.f / (1.f + expf(-(dot + bias)));
            if (e < end) {                         // an edge past the end holds zeros: nothing to add
                if (l == 0) w[e] = gate;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    acc[k].x += x[t][k].x * gate;
                    acc[k].y += x[t][k].y * gate;
                    acc[k].z += x[t][k].z * gate;
                    acc[k].w += x[t][k].w * gate;
                }
            }
        }
    }
    const float deg = (float)max(end - beg, 1);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        float4 s = gr_cross_sum4<G>(acc[k]);
        if (sub == 0 && live[k]) {
            if (reduce_mean) {                     // DGL fn.mean: the sum over the in-degree
                s.x = s.x / deg; s.y = s.y / deg; s.z = s.z / deg; s.w = s.w / deg;
            }
            const float4 hv = *reinterpret_cast<const float4*>(h + (long)v * H + col[k]);
            *reinterpret_cast<float4*>(u + (long)v * H + col[k]) = make_float4(s.x + hv.x, s.y + hv.y, s.z + hv.z, s.w + hv.w);
        }
    }
}

template <int G, int R>
__global__ void __launch_bounds__(256)
gate_reduce_bwd_kernel(const float* __restrict__ gu, const float* __restrict__ m, const float* __restrict__ w,
                       const float* __restrict__ ws, const int* __restrict__ in_ptr, int N, int H, int reduce_mean,
                       float* __restrict__ gm, float* __restrict__ part_ws, float* __restrict__ part_bs) {
    I3D_CHAIN_PRIO();
    constexpr int S = WAVE / G;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    const int lane = threadIdx.x & 63, sub = lane / G, l = lane % G;
    const int beg = in_ptr[v], end = in_ptr[v + 1];
    const float deg = (float)max(end - beg, 1);
    int col[R];
    bool live[R];
    float4 wv[R], g[R], acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        col[k] = l * 4 + k * 256;
        live[k] = col[k] < H;
        wv[k] = live[k] ? *reinterpret_cast<const float4*>(ws + col[k]) : gr_zero();
        g[k] = live[k] ? *reinterpret_cast<const float4*>(gu + (long)v * H + col[k]) : gr_zero();
        if (reduce_mean) {
            g[k].x = g[k].x / deg; g[k].y = g[k].y / deg; g[k].z = g[k].z / deg; g[k].w = g[k].w / deg;
        }
        acc[k] = gr_zero();
    }
    float acc_b = 0.f;
    for (int j0 = beg; j0 < end; j0 += GR_UNROLL * S) {
        float4 x[GR_UNROLL][R];
        float gate[GR_UNROLL];
#pragma unroll
        for (int t = 0; t < GR_UNROLL; ++t) {
            const int e = j0 + t * S + sub;
            gate[t] = e < end ? w[e] : 0.f;
#pragma unroll
            for (int k = 0; k < R; ++k)
                x[t][k] = (e < end && live[k]) ? *reinterpret_cast<const float4*>(m + (long)e * H + col[k]) : gr_zero();
        }
#pragma unroll
        for (int t = 0; t < GR_UNROLL; ++t) {
            const int e = j0 + t * S + sub;
            float dot = gr_dot(g[0], x[t][0]);
#pragma unroll
            for (int k = 1; k < R; ++k) dot += gr_dot(g[k], x[t][k]);
            dot = gr_group_sum<G>(dot);
            const float gg = dot * gate[t] * (1.f - gate[t]);
            if (e < end) {
                if (l == 0) acc_b += gg;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    if (live[k])
                        *reinterpret_cast<float4*>(gm + (long)e * H + col[k]) =
                            make_float4(g[k].x * gate[t] + gg * wv[k].x, g[k].y * gate[t] + gg * wv[k].y,
                                        g[k].z * gate[t] + gg * wv[k].z, g[k].w * gate[t] + gg * wv[k].w);
                    acc[k].x += gg * x[t][k].x;
                    acc[k].y += gg * x[t][k].y;
                    acc[k].z += gg * x[t][k].z;
                    acc[k].w += gg * x[t][k].w;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const float4 s = gr_cross_sum4<G>(acc[k]);
        if (sub == 0 && live[k]) *reinterpret_cast<float4*>(part_ws + (long)v * H + col[k]) = s;
    }
    acc_b = gr_cross_sum<G>(acc_b);                // lanes with l != 0 hold 0
    if (lane == 0) part_bs[v] = acc_b;
}

static bool gr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_gate_reduce_max_feat(void) { return GR_MAX_FEAT; }

#define GR_DISPATCH(KERNEL, ...)                                                                                                   \
    do {                                                                                                                           \
        const dim3 grid_(cdiv(num_nodes, 4)), block_(256);                                                                         \
        hipStream_t s_ = (hipStream_t)stream;                                                                                      \
        if (feat <= 32) hipLaunchKernelGGL((KERNEL<8, 1>), grid_, block_, 0, s_, __VA_ARGS__);                                     \
        else if (feat <= 64) hipLaunchKernelGGL((KERNEL<16, 1>), grid_, block_, 0, s_, __VA_ARGS__);                               \
        else if (feat <= 128) hipLaunchKernelGGL((KERNEL<32, 1>), grid_, block_, 0, s_, __VA_ARGS__);                              \
        else if (feat <= 256) hipLaunchKernelGGL((KERNEL<64, 1>), grid_, block_, 0, s_, __VA_ARGS__);                              \
        else hipLaunchKernelGGL((KERNEL<64, 2>), grid_, block_, 0, s_, __VA_ARGS__);                                               \
    } while (0)

extern "C" int i3d_gate_reduce_fwd(const float* m, const float* ws, const float* bs, const int* in_ptr, const float* h, int num_nodes,
                                   int num_edges, int feat, int reduce_mean, float* u, float* w, void* stream) {
    I3D_CHECK_ARG(num_nodes >= 1, "num_nodes below 1");
    I3D_CHECK_ARG(num_edges >= 0, "num_edges below 0");
    I3D_CHECK_ARG(feat >= 1, "feat below 1");
    if (feat % 4 != 0 || feat > GR_MAX_FEAT) return I3D_NOT_TAKEN;
    I3D_CHECK_ARG(ws && bs && in_ptr && h && u, "null pointer");
    I3D_CHECK_ARG(num_edges == 0 || (m && w), "edges without m / w");
    if (!(gr_aligned16(m) && gr_aligned16(ws) && gr_aligned16(h) && gr_aligned16(u))) return I3D_NOT_TAKEN;
    GR_DISPATCH(gate_reduce_fwd_kernel, m, ws, bs, in_ptr, h, num_nodes, feat, reduce_mean, u, w);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gate_reduce_bwd(const float* gu, const float* m, const float* w, const float* ws, const int* in_ptr, int num_nodes,
                                   int num_edges, int feat, int reduce_mean, float* gm, float* part_ws, float* part_bs, void* stream) {
    I3D_CHECK_ARG(num_nodes >= 1, "num_nodes below 1");
    I3D_CHECK_ARG(num_edges >= 0, "num_edges below 0");
    I3D_CHECK_ARG(feat >= 1, "feat below 1");
    if (feat % 4 != 0 || feat > GR_MAX_FEAT) return I3D_NOT_TAKEN;
    I3D_CHECK_ARG(gu && ws && in_ptr && part_ws && part_bs, "null pointer");
    I3D_CHECK_ARG(num_edges == 0 || (m && w && gm), "edges without m / w / gm");
    if (!(gr_aligned16(gu) && gr_aligned16(m) && gr_aligned16(ws) && gr_aligned16(gm) && gr_aligned16(part_ws))) return I3D_NOT_TAKEN;
    GR_DISPATCH(gate_reduce_bwd_kernel, gu, m, w, ws, in_ptr, num_nodes, feat, reduce_mean, gm, part_ws, part_bs);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
