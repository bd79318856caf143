// GIN message step with edge features (reference models/gin.py:101-108, GINConv.forward, and :276, the virtual-node add), both
// directions, with the bond embedding as a row of the [V, H] table of all feature combinations (ops.edge_codes):
//
//   x[v] = h[v] + vn[graph(v)]                                   (virtual node; x = h without one)
//   z[v] = (1 + eps) x[v] + sum_{e: dst(e) = v} relu(x[src(e)] + T[code(e)])
//
// No [E, H] tensor exists in either direction: the forward is a CSR gather over the in-edges of a node, the backward one over its
// out-edges with the ReLU gate recomputed from x and T (strict >, torch's ReLU backward).  The table (60 rows of H floats, 72 KB
// at H = 300) is read through L2; rows are read whole, by consecutive lanes.
//
//   forward    thread = (node, 4 columns | 1 column): edges of the node in in_ptr order, fp32, one launch.  A source is in the
//              molecule of its destination, so x[src] = h[src] + vn[graph(dst)]: x is written, never read.
//   backward   1. thread = (node u, columns): dx[u] = (1 + eps) g[u] + sum over the out-edges (out_ptr / out_epos order) of
//                 g[dst] gate; the same thread has g[u] and x[u]: its share of <g, x> in fp64 -> one partial per workgroup.
//              2. dT: the per-code edge lists are extremely skewed (most bonds are single, non-ring), so the reduction runs over
//                 FIXED chunks of GIN_CHUNK positions of the code-sorted edge list, whatever codes they hold: workgroup k walks
//                 its positions in order with one fp64 accumulator per column and closes a run whenever the code changes.  Run
//                 (k, c) goes to slot k + c of the partials: along the sorted list neither k nor c decreases and one of them grows
//                 between two runs, so the slots are distinct and there are fewer than chunks + V of them.
//              3. per code the partials of its chunks in chunk order (fp64), rounded once; a code without edges gets a zero row.
//                 One more workgroup sums the <g, x> partials in block order.
//
// Every sum has a fixed order; no atomics; no buffer beyond the caller's.
#include "common.h"

namespace i3d {

constexpr int GIN_CHUNK = 128;            // positions of the code-sorted list per dT workgroup
constexpr int GIN_MAX_BLOCKS = 1 << 16;   // element kernels: grid-stride above this many workgroups
constexpr int GIN_MAX_CODES = 256;

template <int VEC>
__device__ __forceinline__ void gin_load(const float* __restrict__ p, float (&r)[VEC]) {
    if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r[0] = q.x;
        r[1 % VEC] = q.y;
        r[2 % VEC] = q.z;
        r[3 % VEC] = q.w;
    } else {
        r[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void gin_store(float* __restrict__ p, const float (&r)[VEC]) {
    if (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    } else {
        p[0] = r[0];
    }
}

// graph of node v: the b with graph_ptr[b] <= v < graph_ptr[b + 1] (empty graphs skipped)
__device__ __forceinline__ int gin_graph_of(const int* __restrict__ graph_ptr, int num_graphs, int v) {
    int lo = 0, hi = num_graphs;          // graph_ptr[lo] <= v < graph_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (graph_ptr[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

template <int VEC>
__global__ void __launch_bounds__(256)
gin_conv_fwd_kernel(const float* __restrict__ h, const float* __restrict__ vn, const int* __restrict__ graph_ptr, int num_graphs,
                    const float* __restrict__ T, const int* __restrict__ codes, const int* __restrict__ in_ptr,
                    const int* __restrict__ src_s, const float* __restrict__ eps, int N, int H, float* __restrict__ x,
                    float* __restrict__ z) {
    I3D_CHAIN_PRIO();
    const int HV = H / VEC;
    const long total = (long)N * HV;
    const float scale = 1.f + eps[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int v = (int)(i / HV), c = (int)(i - (long)v * HV) * VEC;
        float xv[VEC], add[VEC], acc[VEC];
        gin_load<VEC>(h + (long)v * H + c, xv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) add[k] = 0.f;
        if (vn) {
            gin_load<VEC>(vn + (long)gin_graph_of(graph_ptr, num_graphs, v) * H + c, add);
#pragma unroll
            for (int k = 0; k < VEC; ++k) xv[k] = xv[k] + add[k];
            gin_store<VEC>(x + (long)v * H + c, xv);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        const int e1 = in_ptr[v + 1];
        for (int e = in_ptr[v]; e < e1; ++e) {
            float xs[VEC], t[VEC];
            gin_load<VEC>(h + (long)src_s[e] * H + c, xs);
            gin_load<VEC>(T + (long)codes[e] * H + c, t);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float m = (vn ? xs[k] + add[k] : xs[k]) + t[k];
                acc[k] = acc[k] + (m > 0.f ? m : 0.f);
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = scale * xv[k] + acc[k];
        gin_store<VEC>(z + (long)v * H + c, acc);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
gin_conv_bwd_dx_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ T,
                       const int* __restrict__ codes, const int* __restrict__ dst_s, const int* __restrict__ out_ptr,
                       const int* __restrict__ out_epos, const float* __restrict__ eps, int N, int H, float* __restrict__ dx,
                       double* __restrict__ deps_partial) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int HV = H / VEC;
    const long total = (long)N * HV;
    const float scale = 1.f + eps[0];
    double dot = 0.;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int u = (int)(i / HV), c = (int)(i - (long)u * HV) * VEC;
        float xu[VEC], gu[VEC], acc[VEC];
        gin_load<VEC>(x + (long)u * H + c, xu);
        gin_load<VEC>(g + (long)u * H + c, gu);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dot += (double)gu[k] * (double)xu[k];
            acc[k] = 0.f;
        }
        const int j1 = out_ptr[u + 1];
        for (int j = out_ptr[u]; j < j1; ++j) {
            const int e = out_epos[j];
            float gd[VEC], t[VEC];
            gin_load<VEC>(g + (long)dst_s[e] * H + c, gd);
            gin_load<VEC>(T + (long)codes[e] * H + c, t);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + (xu[k] + t[k] > 0.f ? gd[k] : 0.f);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = scale * gu[k] + acc[k];
        gin_store<VEC>(dx + (long)u * H + c, acc);
    }
    dot = block_sum_f64(dot, sm);
    if (threadIdx.x == 0) deps_partial[blockIdx.x] = dot;
}

// workgroup (k, column tile): positions [k GIN_CHUNK, (k + 1) GIN_CHUNK) of the code-sorted list, thread = one column
__global__ void __launch_bounds__(256)
gin_conv_bwd_dT_chunk_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ T,
                             const int* __restrict__ codes, const int* __restrict__ src_s, const int* __restrict__ dst_s,
                             const int* __restrict__ order, int E, int H, double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ int s_src[GIN_CHUNK], s_dst[GIN_CHUNK], s_code[GIN_CHUNK];
    const int p0 = blockIdx.x * GIN_CHUNK, n = min(GIN_CHUNK, E - p0);
    for (int i = threadIdx.x; i < n; i += 256) {
        const int e = order[p0 + i];
        s_src[i] = src_s[e];
        s_dst[i] = dst_s[e];
        s_code[i] = codes[e];
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= H) return;
    int code = s_code[0];
    float t = T[(long)code * H + c];
    double acc = 0.;
    for (int i = 0; i < n; ++i) {
        const int ci = s_code[i];
        if (ci != code) {
            partial[((long)blockIdx.x + code) * H + c] = acc;
            code = ci;
            t = T[(long)code * H + c];
            acc = 0.;
        }
        const float xu = x[(long)s_src[i] * H + c], gd = g[(long)s_dst[i] * H + c];
        acc += (xu + t > 0.f) ? (double)gd : 0.;
    }
    partial[((long)blockIdx.x + code) * H + c] = acc;
}

// workgroups 0..V-1: dT row of one code from the partials of its chunks; workgroup V: deps from the per-workgroup partials
__global__ void __launch_bounds__(256)
gin_conv_bwd_final_kernel(const double* __restrict__ partial, const int* __restrict__ code_ptr, int V, int H,
                          const double* __restrict__ deps_partial, int deps_blocks, float* __restrict__ dT, float* __restrict__ deps) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    if ((int)blockIdx.x == V) {
        double s = 0.;
        for (int b = threadIdx.x; b < deps_blocks; b += 256) s += deps_partial[b];
        s = block_sum_f64(s, sm);
        if (threadIdx.x == 0) deps[0] = (float)s;
        return;
    }
    const int code = blockIdx.x, a = code_ptr[code], b = code_ptr[code + 1];
    for (int c = threadIdx.x; c < H; c += 256) {
        double s = 0.;
        if (b > a) {
            const int k1 = (b - 1) / GIN_CHUNK;
            for (int k = a / GIN_CHUNK; k <= k1; ++k) s += partial[((long)k + code) * H + c];
        }
        dT[(long)code * H + c] = (float)s;
    }
}

static int gin_blocks(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > GIN_MAX_BLOCKS ? GIN_MAX_BLOCKS : b));
}

static bool gin_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace i3d

using namespace i3d;

static int gin_check(int num_nodes, int num_edges, int feat, int num_codes) {
    I3D_CHECK_ARG(num_nodes >= 1, "num_nodes below 1");
    I3D_CHECK_ARG(num_edges >= 0, "num_edges below 0");
    I3D_CHECK_ARG(feat >= 1, "feat below 1");
    I3D_CHECK_ARG(num_codes >= 1 && num_codes <= GIN_MAX_CODES, "num_codes outside 1..256");
    return I3D_OK;
}

extern "C" int i3d_gin_chunk_edges(void) { return GIN_CHUNK; }

extern "C" long i3d_gin_conv_bwd_partial_floats(int num_nodes, int num_edges, int feat, int num_codes) {
    if (num_nodes < 1 || num_edges < 0 || feat < 1 || num_codes < 1 || num_codes > GIN_MAX_CODES) return 0;
    const long chunks = ((long)num_edges + GIN_CHUNK - 1) / GIN_CHUNK;
    return 2L * ((chunks + num_codes) * feat + GIN_MAX_BLOCKS);        // fp64 each
}

extern "C" int i3d_gin_conv_fwd(const float* h, const float* vn, const int* graph_ptr, int num_graphs, const float* T, int num_codes,
                                const int* codes, const int* in_ptr, const int* src_s, const float* eps, int num_nodes,
                                int num_edges, int feat, float* x, float* z, void* stream) {
    if (int rc = gin_check(num_nodes, num_edges, feat, num_codes)) return rc;
    I3D_CHECK_ARG(h && T && in_ptr && eps && z, "null pointer");
    I3D_CHECK_ARG(num_edges == 0 || (codes && src_s), "edges without codes / src_s");
    I3D_CHECK_ARG(!vn || (graph_ptr && num_graphs >= 1 && x), "vn without graph_ptr / num_graphs / x");
    const bool vec = feat % 4 == 0 && gin_aligned16(h) && gin_aligned16(T) && gin_aligned16(z) && (!vn || (gin_aligned16(vn) && gin_aligned16(x)));
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        hipLaunchKernelGGL(gin_conv_fwd_kernel<4>, dim3(gin_blocks((long)num_nodes * (feat / 4))), dim3(256), 0, s, h, vn, graph_ptr,
                           num_graphs, T, codes, in_ptr, src_s, eps, num_nodes, feat, x, z);
    } else {
        hipLaunchKernelGGL(gin_conv_fwd_kernel<1>, dim3(gin_blocks((long)num_nodes * feat)), dim3(256), 0, s, h, vn, graph_ptr,
                           num_graphs, T, codes, in_ptr, src_s, eps, num_nodes, feat, x, z);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_gin_conv_bwd(const float* g, const float* x, const float* T, int num_codes, const int* codes, const int* src_s,
                                const int* dst_s, const int* out_ptr, const int* out_epos, const int* code_order,
                                const int* code_ptr, const float* eps, int num_nodes, int num_edges, int feat, float* partials,
                                float* dx, float* dT, float* deps, void* stream) {
    if (int rc = gin_check(num_nodes, num_edges, feat, num_codes)) return rc;
    I3D_CHECK_ARG(g && x && T && out_ptr && code_ptr && eps && partials && dx && dT && deps, "null pointer");
    I3D_CHECK_ARG(num_edges == 0 || (codes && src_s && dst_s && out_epos && code_order), "edges without their index arrays");
    I3D_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "partials not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = cdiv(num_edges, GIN_CHUNK);
    double* part = reinterpret_cast<double*>(partials);
    double* deps_part = part + ((long)chunks + num_codes) * feat;
    const bool vec = feat % 4 == 0 && gin_aligned16(g) && gin_aligned16(x) && gin_aligned16(T) && gin_aligned16(dx);
    const int blocks = gin_blocks((long)num_nodes * (vec ? feat / 4 : feat));
    if (vec) {
        hipLaunchKernelGGL(gin_conv_bwd_dx_kernel<4>, dim3(blocks), dim3(256), 0, s, g, x, T, codes, dst_s, out_ptr, out_epos, eps,
                           num_nodes, feat, dx, deps_part);
    } else {
        hipLaunchKernelGGL(gin_conv_bwd_dx_kernel<1>, dim3(blocks), dim3(256), 0, s, g, x, T, codes, dst_s, out_ptr, out_epos, eps,
                           num_nodes, feat, dx, deps_part);
    }
    I3D_CHECK_LAUNCH();
    if (chunks > 0) {
        hipLaunchKernelGGL(gin_conv_bwd_dT_chunk_kernel, dim3(chunks, cdiv(feat, 256)), dim3(256), 0, s, g, x, T, codes, src_s, dst_s,
                           code_order, num_edges, feat, part);
        I3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(gin_conv_bwd_final_kernel, dim3(num_codes + 1), dim3(256), 0, s, (const double*)part, code_ptr, num_codes, feat,
                       (const double*)deps_part, blocks, dT, deps);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
