// GeoMol's message-passing step (reference models/geomol_mpnn.py: EdgeModel.forward :93-99, GeomolMetaLayer.forward :72-74), the parts
// that are not a dense product.  Every edge tensor is in destination-sorted order (graph.GraphIndex).
//
//   edge forward    h[j] = relu(F[j] + P[src(j)] + Q[dst(j)])                F [E, H] = edge(e) with its bias, P | Q the two halves
//                                                                            of the rows of ONE [N, 2H] product x [W_in | W_out]^T
//   edge backward   dF[j] = g[j] [h[j] > 0];  dP[u] = sum of dF over the out-edges of u;  dQ[v] = sum of dF over the in-edges of v
//   residual        out = (1 + eps) a + b  and its backward  da = (1 + eps) g,  deps = <g, a>   (edges and nodes both: eps is
//                                                                            edge_eps or node_eps, read from device memory)
//
//   edge forward    thread = (edge, 4 columns | 1 column); the rows of P and Q are read whole by consecutive lanes, through L2
//                   (a node's row is read by its ~2 out-edges and ~2 in-edges).
//   edge backward   ONE launch, thread = (node v, 4 columns | 1 column).  The thread walks the in-edges of v (in_ptr order: rows
//                   in_ptr[v] .. in_ptr[v + 1] of g and h are contiguous), forms dF[j], stores it - every edge has one destination,
//                   so dF is written exactly once - and adds it to dQ[v]; then it walks the out-edges of v (out_ptr / out_epos
//                   order), forms the same value again from g and h (never from the dF another thread is writing) and adds it to
//                   dP[v].  g and h are read twice, the second time from L2; nothing is read that this launch writes.  A node
//                   without in-edges (out-edges) stores a zero row.  dP | dQ are the halves of one [N, 2H] buffer.
//   residual bwd    da elementwise; the thread's share of <g, a> in fp64 -> one partial per workgroup, summed in workgroup order by
//                   a second, one-workgroup launch and rounded once (as gin.hip does for its eps).
//
// Every sum has a fixed order; no atomics; no buffer beyond the caller's.  16-byte accesses when H % 4 == 0 and the buffers are
// 16-byte aligned, else one float at a time (H = 50, the width of configs/geomolgnn_wrapper_ogb_feat.yml, takes that path).
#include "common.h"

namespace i3d {

constexpr int GEOMOL_MAX_BLOCKS = 1 << 16;                                // element kernels: grid-stride above this many workgroups
constexpr int GEOMOL_EPS_BLOCKS = I3D_GEOMOL_PARTIAL_FLOATS / 2;          // residual backward: one fp64 partial per workgroup

template <int VEC>
__device__ __forceinline__ void geomol_load(const float* __restrict__ p, float (&r)[VEC]) {
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
__device__ __forceinline__ void geomol_store(float* __restrict__ p, const float (&r)[VEC]) {
    if (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
    } else {
        p[0] = r[0];
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
geomol_edge_fwd_kernel(const float* __restrict__ F, const float* __restrict__ PQ, const int* __restrict__ src_s,
                       const int* __restrict__ dst_s, int E, int H, float* __restrict__ h) {
    I3D_CHAIN_PRIO();
    const int HV = H / VEC;
    const long total = (long)E * HV;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i / HV), c = (int)(i - (long)j * HV) * VEC;
        float f[VEC], p[VEC], q[VEC];
        geomol_load<VEC>(F + (long)j * H + c, f);
        geomol_load<VEC>(PQ + (long)src_s[j] * 2 * H + c, p);
        geomol_load<VEC>(PQ + (long)dst_s[j] * 2 * H + H + c, q);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float m = (f[k] + p[k]) + q[k];
            f[k] = m > 0.f ? m : 0.f;
        }
        geomol_store<VEC>(h + (long)j * H + c, f);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
geomol_edge_bwd_kernel(const float* __restrict__ g, const float* __restrict__ h, const int* __restrict__ in_ptr,
                       const int* __restrict__ out_ptr, const int* __restrict__ out_epos, int N, int H, float* __restrict__ dF,
                       float* __restrict__ dPQ) {
    I3D_CHAIN_PRIO();
    const int HV = H / VEC;
    const long total = (long)N * HV;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int v = (int)(i / HV), c = (int)(i - (long)v * HV) * VEC;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        const int e1 = in_ptr[v + 1];
        for (int j = in_ptr[v]; j < e1; ++j) {
            float gj[VEC], hj[VEC];
            geomol_load<VEC>(g + (long)j * H + c, gj);
            geomol_load<VEC>(h + (long)j * H + c, hj);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                gj[k] = hj[k] > 0.f ? gj[k] : 0.f;
                acc[k] = acc[k] + gj[k];
            }
            geomol_store<VEC>(dF + (long)j * H + c, gj);
        }
        geomol_store<VEC>(dPQ + (long)v * 2 * H + H + c, acc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        const int o1 = out_ptr[v + 1];
        for (int o = out_ptr[v]; o < o1; ++o) {
            const int j = out_epos[o];
            float gj[VEC], hj[VEC];
            geomol_load<VEC>(g + (long)j * H + c, gj);
            geomol_load<VEC>(h + (long)j * H + c, hj);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + (hj[k] > 0.f ? gj[k] : 0.f);
        }
        geomol_store<VEC>(dPQ + (long)v * 2 * H + c, acc);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
geomol_residual_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ eps, long n,
                           float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    const float scale = 1.f + eps[0];
    const long total = n / VEC;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float av[VEC], bv[VEC];
        geomol_load<VEC>(a + i * VEC, av);
        geomol_load<VEC>(b + i * VEC, bv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) av[k] = scale * av[k] + bv[k];
        geomol_store<VEC>(out + i * VEC, av);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256)
geomol_residual_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ eps, long n,
                           float* __restrict__ da, double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const float scale = 1.f + eps[0];
    const long total = n / VEC;
    double dot = 0.;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float gv[VEC], av[VEC];
        geomol_load<VEC>(g + i * VEC, gv);
        geomol_load<VEC>(a + i * VEC, av);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dot += (double)gv[k] * (double)av[k];
            gv[k] = scale * gv[k];
        }
        geomol_store<VEC>(da + i * VEC, gv);
    }
    dot = block_sum_f64(dot, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = dot;
}

// one workgroup: the per-workgroup partials in workgroup order, rounded once
__global__ void __launch_bounds__(256)
geomol_residual_bwd_final_kernel(const double* __restrict__ partial, int blocks, float* __restrict__ deps) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double s = 0.;
    for (int b = threadIdx.x; b < blocks; b += 256) s += partial[b];
    s = block_sum_f64(s, sm);
    if (threadIdx.x == 0) deps[0] = (float)s;
}

static int geomol_blocks(long total, int cap) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

static bool geomol_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace i3d

using namespace i3d;

static int geomol_check(int num_nodes, int num_edges, int feat) {
    I3D_CHECK_ARG(num_nodes >= 1, "num_nodes below 1");
    I3D_CHECK_ARG(num_edges >= 0, "num_edges below 0");
    I3D_CHECK_ARG(feat >= 1, "feat below 1");
    return I3D_OK;
}

extern "C" int i3d_geomol_edge_fwd(const float* F, const float* PQ, const int* src_s, const int* dst_s, int num_nodes, int num_edges,
                                   int feat, float* h, void* stream) {
    if (int rc = geomol_check(num_nodes, num_edges, feat)) return rc;
    I3D_CHECK_ARG(PQ, "null pointer");
    if (num_edges == 0) return I3D_OK;
    I3D_CHECK_ARG(F && src_s && dst_s && h, "edges without F / src_s / dst_s / h");
    hipStream_t s = (hipStream_t)stream;
    if (feat % 4 == 0 && geomol_aligned16(F) && geomol_aligned16(PQ) && geomol_aligned16(h)) {
        hipLaunchKernelGGL(geomol_edge_fwd_kernel<4>, dim3(geomol_blocks((long)num_edges * (feat / 4), GEOMOL_MAX_BLOCKS)), dim3(256),
                           0, s, F, PQ, src_s, dst_s, num_edges, feat, h);
    } else {
        hipLaunchKernelGGL(geomol_edge_fwd_kernel<1>, dim3(geomol_blocks((long)num_edges * feat, GEOMOL_MAX_BLOCKS)), dim3(256), 0, s,
                           F, PQ, src_s, dst_s, num_edges, feat, h);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_geomol_edge_bwd(const float* g, const float* h, const int* in_ptr, const int* out_ptr, const int* out_epos,
                                   int num_nodes, int num_edges, int feat, float* dF, float* dPQ, void* stream) {
    if (int rc = geomol_check(num_nodes, num_edges, feat)) return rc;
    I3D_CHECK_ARG(in_ptr && out_ptr && dPQ, "null pointer");
    I3D_CHECK_ARG(num_edges == 0 || (g && h && out_epos && dF), "edges without g / h / out_epos / dF");
    hipStream_t s = (hipStream_t)stream;
    if (feat % 4 == 0 && geomol_aligned16(g) && geomol_aligned16(h) && geomol_aligned16(dF) && geomol_aligned16(dPQ)) {
        hipLaunchKernelGGL(geomol_edge_bwd_kernel<4>, dim3(geomol_blocks((long)num_nodes * (feat / 4), GEOMOL_MAX_BLOCKS)), dim3(256),
                           0, s, g, h, in_ptr, out_ptr, out_epos, num_nodes, feat, dF, dPQ);
    } else {
        hipLaunchKernelGGL(geomol_edge_bwd_kernel<1>, dim3(geomol_blocks((long)num_nodes * feat, GEOMOL_MAX_BLOCKS)), dim3(256), 0, s,
                           g, h, in_ptr, out_ptr, out_epos, num_nodes, feat, dF, dPQ);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

static int geomol_residual_check(long rows, int feat) {
    I3D_CHECK_ARG(rows >= 0, "rows below 0");
    I3D_CHECK_ARG(feat >= 1, "feat below 1");
    return I3D_OK;
}

extern "C" int i3d_geomol_residual_fwd(const float* a, const float* b, const float* eps, long rows, int feat, float* out,
                                       void* stream) {
    if (int rc = geomol_residual_check(rows, feat)) return rc;
    I3D_CHECK_ARG(eps, "null pointer");
    const long n = rows * feat;
    if (n == 0) return I3D_OK;
    I3D_CHECK_ARG(a && b && out, "rows without a / b / out");
    hipStream_t s = (hipStream_t)stream;
    if (n % 4 == 0 && geomol_aligned16(a) && geomol_aligned16(b) && geomol_aligned16(out)) {
        hipLaunchKernelGGL(geomol_residual_fwd_kernel<4>, dim3(geomol_blocks(n / 4, GEOMOL_MAX_BLOCKS)), dim3(256), 0, s, a, b, eps, n,
                           out);
    } else {
        hipLaunchKernelGGL(geomol_residual_fwd_kernel<1>, dim3(geomol_blocks(n, GEOMOL_MAX_BLOCKS)), dim3(256), 0, s, a, b, eps, n, out);
    }
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_geomol_residual_bwd(const float* g, const float* a, const float* eps, long rows, int feat, float* partials,
                                       float* da, float* deps, void* stream) {
    if (int rc = geomol_residual_check(rows, feat)) return rc;
    I3D_CHECK_ARG(eps && partials && deps, "null pointer");
    I3D_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "partials not 8-byte aligned");
    const long n = rows * feat;
    I3D_CHECK_ARG(n == 0 || (g && a && da), "rows without g / a / da");
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(partials);
    int blocks = 0;
    if (n > 0) {
        if (n % 4 == 0 && geomol_aligned16(g) && geomol_aligned16(a) && geomol_aligned16(da)) {
            blocks = geomol_blocks(n / 4, GEOMOL_EPS_BLOCKS);
            hipLaunchKernelGGL(geomol_residual_bwd_kernel<4>, dim3(blocks), dim3(256), 0, s, g, a, eps, n, da, part);
        } else {
            blocks = geomol_blocks(n, GEOMOL_EPS_BLOCKS);
            hipLaunchKernelGGL(geomol_residual_bwd_kernel<1>, dim3(blocks), dim3(256), 0, s, g, a, eps, n, da, part);
        }
        I3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(geomol_residual_bwd_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, blocks, deps);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
