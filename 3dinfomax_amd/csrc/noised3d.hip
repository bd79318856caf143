// Device-side construction of the (1 + U)-fold noised complete-graph batch of the noised-3D negatives (reference
// datasets/custom_collate.py:131-152 NoisedDistancesCollate, :160-185 NoisedCoordinatesCollate; consumer: NTXentExtraNegatives,
// csrc/hardneg.hip).
//
// The reference deep-copies the batched 3D graph U times on the host, noises each copy and batches the 1 + U graphs.  Everything
// about those copies is analytic: the structure is the clean batch's (closed forms at the top of batch.hip) with molecule
// c B + g offset by c N nodes and c E3 edges, the distances are the clean ones plus noise.  So one launch writes the whole batch
// from what the clean batch uploads anyway: coords [N, 3], graph_ptr [B + 1], edge_ptr [B + 1].  No copy of the clean arrays is
// read back.
//
// Thread map: blockIdx.y = copy c, t = position inside the copy.  For molecule g (n atoms, offsets nb / eb) and t = eb + a (n-1) + j,
// b = j < a ? j : j + 1, mirror = eb + b (n-1) + (a < b ? a : a - 1):
//   as EDGE ID t   the edge is a -> b: src / dst / d / inv_perm / out_epos [t], epos = mirror
//   as EPOS    t   the edge is b -> a: src_s / dst_s / perm [t],               id   = mirror
// so every store of the launch goes to index c E3 + t: all of them coalesce, every element has exactly one writer, no atomics.
//
// Noise: counter-based (Philox4x32-10), key = the two words of a 64-bit seed, counter = (element, copy, step_lo, step_hi), element =
// the clean batch's edge id (distances mode) or node id (coordinates mode) - independent of the launch geometry and recomputable
// anywhere, so no [U, N, 3] tensor is stored: in coordinates mode both ends of an edge recompute their node's 3-vector, and both
// directions of a pair see the same positions.  u(w) = fl32(((w >> 8) + 0.5) 2^-24) in (0, 1]; z0 = sqrt(-2 ln u(w0)) cos(2 pi u(w1)),
// z1 the sine partner, z2 = sqrt(-2 ln u(w2)) cos(2 pi u(w3)).  tests/noise_reference.py is the host mirror.
#include "common.h"

namespace i3d {

__device__ __forceinline__ int nz_find_graph(const int* __restrict__ ptr, int num_graphs, int x) {
    int lo = 0, hi = num_graphs;          // ptr[lo] <= x < ptr[hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (ptr[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

__device__ __forceinline__ float nz_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 0x1p-24f; }

__device__ __forceinline__ float nz_radius(uint32_t w) { return sqrtf(-2.f * logf(nz_uniform(w))); }

struct NoiseKey {
    uint32_t k0, k1, s0, s1;      // seed and step words
};

// z0 of (element, copy): the one normal an edge takes in distances mode
__device__ __forceinline__ float nz_normal1(uint32_t element, uint32_t copy, const NoiseKey& k) {
    uint32_t w[4];
    philox4x32_10(element, copy, k.s0, k.s1, k.k0, k.k1, w);
    return nz_radius(w[0]) * cospif(2.f * nz_uniform(w[1]));
}

// coords[node] + std (z0, z1, z2) of (node, copy); copy 0 is the clean position
__device__ __forceinline__ void nz_position(const float* __restrict__ coords, int node, uint32_t copy, float std_,
                                            const NoiseKey& k, float p[3]) {
    const float* a = coords + (long)node * 3;
    p[0] = a[0], p[1] = a[1], p[2] = a[2];
    if (copy == 0) return;
    uint32_t w[4];
    philox4x32_10((uint32_t)node, copy, k.s0, k.s1, k.k0, k.k1, w);
    float s, c;
    sincospif(2.f * nz_uniform(w[1]), &s, &c);
    const float r = nz_radius(w[0]);
    p[0] = p[0] + std_ * (r * c);
    p[1] = p[1] + std_ * (r * s);
    p[2] = p[2] + std_ * (nz_radius(w[2]) * cospif(2.f * nz_uniform(w[3])));
}

template <bool COORDS>
__global__ void __launch_bounds__(256)
noised_graph_kernel(const float* __restrict__ coords, const int* __restrict__ graph_ptr, const int* __restrict__ edge_ptr,
                    int num_graphs, int num_nodes, int num_edges, float std_, NoiseKey key, int* __restrict__ in_ptr,
                    int* __restrict__ src_s, int* __restrict__ dst_s, int* __restrict__ perm, int* __restrict__ inv_perm,
                    int* __restrict__ out_epos, int* __restrict__ graph_ptr_out, int64_t* __restrict__ src_id,
                    int64_t* __restrict__ dst_id, float* __restrict__ d_id, float* __restrict__ x_out) {
    I3D_CHAIN_PRIO();
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    const bool last = c == (int)gridDim.y - 1;
    // the host refused totals beyond int32: these products fit
    const int node_off = (int)((long)c * num_nodes), edge_off = (int)((long)c * num_edges);
    if (t < num_graphs) graph_ptr_out[c * num_graphs + t] = node_off + graph_ptr[t];
    if (t == num_graphs && last) graph_ptr_out[c * num_graphs + t] = node_off + num_nodes;
    if (t < num_nodes) {      // node-level: CSR row pointer (identical by destination and by source), the noised positions
        const int g = nz_find_graph(graph_ptr, num_graphs, t);
        const int nb = graph_ptr[g], n = graph_ptr[g + 1] - nb;
        in_ptr[node_off + t] = edge_off + edge_ptr[g] + (t - nb) * (n - 1);
        if (COORDS) {
            float p[3];
            nz_position(coords, t, (uint32_t)c, std_, key, p);
            float* x = x_out + (long)(node_off + t) * 3;
            x[0] = p[0], x[1] = p[1], x[2] = p[2];
        }
    }
    if (t == num_nodes && last) in_ptr[node_off + t] = edge_off + num_edges;
    if (t >= num_edges) return;
    const int g = nz_find_graph(edge_ptr, num_graphs, t);
    const int nb = graph_ptr[g], n = graph_ptr[g + 1] - nb, eb = edge_ptr[g];
    const int loc = t - eb;
    const int a = loc / (n - 1), j = loc - a * (n - 1);
    const int b = j < a ? j : j + 1;
    const int mirror = edge_off + eb + b * (n - 1) + (a < b ? a : a - 1);
    const int na = node_off + nb + a, nd = node_off + nb + b;
    float dist;
    if (COORDS) {
        float pa[3], pb[3];
        nz_position(coords, nb + a, (uint32_t)c, std_, key, pa);
        nz_position(coords, nb + b, (uint32_t)c, std_, key, pb);
        const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
        dist = sqrtf(dx * dx + dy * dy + dz * dz);
    } else {
        const float* pa = coords + (long)(nb + a) * 3;
        const float* pb = coords + (long)(nb + b) * 3;
        const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
        dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (c > 0) dist = dist + std_ * nz_normal1((uint32_t)t, (uint32_t)c, key);      // no clamp, as in the reference
    }
    const long e = (long)edge_off + t;
    // edge id e: a -> b
    src_id[e] = na;
    dst_id[e] = nd;
    d_id[e] = dist;
    inv_perm[e] = mirror;
    out_epos[e] = mirror;
    // epos e: b -> a
    src_s[e] = nd;
    dst_s[e] = na;
    perm[e] = mirror;
}

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_noised_graph_build(const float* coords, const int* graph_ptr, const int* edge_ptr, int num_graphs,
                                      int num_nodes, int num_edges, int num_noised, int mode, float std_,
                                      unsigned long long seed, unsigned long long step, int* in_ptr, int* src_s, int* dst_s,
                                      int* perm, int* inv_perm, int* out_epos, int* graph_ptr_out, int64_t* src_id,
                                      int64_t* dst_id, float* d_id, float* x_out, void* stream) {
    I3D_CHECK_ARG(num_graphs > 0 && num_nodes > 0 && num_edges >= 0, "bad shape");
    I3D_CHECK_ARG(num_noised >= 0 && num_noised < 65535, "num_noised outside 0 .. 65534");
    I3D_CHECK_ARG(mode == I3D_NOISED_DISTANCES || mode == I3D_NOISED_COORDINATES, "mode: distances (0) or coordinates (1)");
    const long copies = 1 + (long)num_noised;
    I3D_CHECK_ARG(copies * (long)num_edges <= 2147483647L && copies * (long)num_nodes + 1 <= 2147483647L,
                  "(1 + num_noised) x the batch does not fit the int32 index arrays");
    I3D_CHECK_ARG(mode == I3D_NOISED_DISTANCES || x_out != nullptr, "coordinates mode writes x: x_out is null");
    int items = num_edges > num_nodes + 1 ? num_edges : num_nodes + 1;
    if (num_graphs + 1 > items) items = num_graphs + 1;
    const NoiseKey key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
    const dim3 grid(cdiv(items, 256), (unsigned)copies);
    if (mode == I3D_NOISED_COORDINATES)
        hipLaunchKernelGGL(noised_graph_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, coords, graph_ptr, edge_ptr,
                           num_graphs, num_nodes, num_edges, std_, key, in_ptr, src_s, dst_s, perm, inv_perm, out_epos,
                           graph_ptr_out, src_id, dst_id, d_id, x_out);
    else
        hipLaunchKernelGGL(noised_graph_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, coords, graph_ptr, edge_ptr,
                           num_graphs, num_nodes, num_edges, std_, key, in_ptr, src_s, dst_s, perm, inv_perm, out_epos,
                           graph_ptr_out, src_id, dst_id, d_id, x_out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
