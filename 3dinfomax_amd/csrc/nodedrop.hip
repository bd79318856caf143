// Node-dropped views of a batch built on the device (the GraphCL baseline's NodeDropCollate, reference
// datasets/custom_collate.py:230-263, with DGL's remove_nodes semantics).
//
// The input is a batch as FlatMolDataset.assemble_host / host_batch_to_device put it on the device: block-diagonal, so
// molecule g owns the contiguous node range [nb, nb+n), and its edge ids, its destination-sorted positions (epos) and its
// out-edge slots are all the same contiguous range [eb, eb+e) with eb = in_ptr[nb].  Removing nodes keeps the order of
// everything that is left, so every array of a view is the old one restricted to what is kept, renumbered:
//   nodes    kept nodes in ascending id                -> new id nb' + rank
//   edge ids kept edges (both ends kept) in id order   -> new id eb' + rank       (src, dst, bond features)
//   epos     kept edges in the old epos order          -> new epos eb' + rank     (perm, src_s, dst_s, inv_perm, in_ptr)
//   out slot kept entries of the old out_epos sequence -> out_epos, out_ptr       (sorted by (src, epos) before and after)
// Each rank is a prefix count inside the molecule: one wave per (molecule, view) takes 64 items at a time, __ballot of the
// keep predicate and mbcnt give every lane its rank, popcount the running base.  The per-molecule output offsets (nb', eb')
// and the slot of every (molecule, in-degree) in deg_rows come from the host, which counted them from the same keep mask:
// no global scan, no atomics (the build is bit-deterministic), no inter-workgroup waits.  Each count is checked against the
// host's before anything is written.
#include "common.h"

namespace i3d {
namespace {

struct NodeDropViews {
    I3dNodeDropView v[2];
};

// number of set bits of m below this lane
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ void __launch_bounds__(64)
node_drop_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const int64_t* __restrict__ atom_feat,
                 const int64_t* __restrict__ bond_feat, const int* __restrict__ in_ptr, const int* __restrict__ perm,
                 const int* __restrict__ src_s, const int* __restrict__ dst_s, const int* __restrict__ out_ptr,
                 const int* __restrict__ out_epos, const int* __restrict__ graph_ptr, int atom_cols, int bond_cols,
                 int max_atoms, int max_edges, int deg_stride, NodeDropViews views) {
    I3D_CHAIN_PRIO();
    extern __shared__ int lds[];
    const I3dNodeDropView& V = views.v[blockIdx.y];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int nb = graph_ptr[g], n = graph_ptr[g + 1] - nb;
    const int eb = in_ptr[nb], ne = in_ptr[nb + n] - eb;
    const int nb2 = V.graph_ptr[g], n2 = V.graph_ptr[g + 1] - nb2;
    const int eb2 = V.edge_ptr[g], ne2 = V.edge_ptr[g + 1] - eb2;

    if (g == 0) {       // the views' last row pointers and the -1 padding of the degree groups
        if (lane == 0) {
            V.in_ptr[V.num_nodes] = V.num_edges;
            V.out_ptr[V.num_nodes] = V.num_edges;
        }
        for (int q = 0; q < V.n_groups; ++q)
            for (int t = V.pad_range[2 * q] + lane; t < V.pad_range[2 * q + 1]; t += WAVE) V.deg_rows[t] = -1;
    }
    if (n < 0 || ne < 0 || n > max_atoms || ne > max_edges) return;     // (the host sized the LDS from these bounds)
    int* nmap = lds;                        // [max_atoms]     local node id -> new node id, -1 removed
    int* emap = nmap + max_atoms;           // [max_edges]     local edge id -> new edge id, -1 removed
    int* erank = emap + max_edges;          // [max_edges + 1] kept edges in front of each local epos
    int* orank = erank + max_edges + 1;     // [max_edges + 1] kept entries in front of each local out slot

    // nodes
    int base = 0;
    for (int c = 0; c < n; c += WAVE) {
        const int i = c + lane;
        const bool k = i < n && V.keep[nb + i] != 0;
        const unsigned long long m = __ballot(k);
        if (i < n) nmap[i] = k ? nb2 + base + lanes_below(m) : -1;
        base += __popcll(m);
    }
    if (base != n2) return;                 // the host's count disagrees: write nothing
    __syncthreads();
    // edges in id order: kept iff both ends are
    base = 0;
    for (int c = 0; c < ne; c += WAVE) {
        const int x = c + lane;
        bool k = false;
        if (x < ne) {
            const unsigned s = (unsigned)(src[eb + x] - nb), d = (unsigned)(dst[eb + x] - nb);
            k = s < (unsigned)n && d < (unsigned)n && nmap[s] >= 0 && nmap[d] >= 0;
        }
        const unsigned long long m = __ballot(k);
        if (x < ne) emap[x] = k ? eb2 + base + lanes_below(m) : -1;
        base += __popcll(m);
    }
    if (base != ne2) return;
    __syncthreads();
    for (int t = lane; t < n * atom_cols; t += WAVE) {
        const int i = t / atom_cols, id = nmap[i];
        if (id >= 0) V.atom_feat[(long)id * atom_cols + (t - i * atom_cols)] = atom_feat[(long)nb * atom_cols + t];
    }
    for (int x = lane; x < ne; x += WAVE) {
        const int id = emap[x];
        if (id >= 0) {
            V.src[id] = nmap[src[eb + x] - nb];
            V.dst[id] = nmap[dst[eb + x] - nb];
        }
    }
    for (int t = lane; t < ne * bond_cols; t += WAVE) {
        const int x = t / bond_cols, id = emap[x];
        if (id >= 0) V.bond_feat[(long)id * bond_cols + (t - x * bond_cols)] = bond_feat[(long)eb * bond_cols + t];
    }
    // edges in epos order (an edge is kept iff its id is)
    base = 0;
    for (int c = 0; c < ne; c += WAVE) {
        const int e = c + lane;
        int id = -1;
        if (e < ne) {
            const unsigned x = (unsigned)(perm[eb + e] - eb);
            id = x < (unsigned)ne ? emap[x] : -1;
        }
        const unsigned long long m = __ballot(id >= 0);
        const int r = base + lanes_below(m);
        if (e < ne) erank[e] = r;
        if (id >= 0) {
            const int ep = eb2 + r;
            V.perm[ep] = id;
            V.inv_perm[id] = ep;
            V.src_s[ep] = nmap[src_s[eb + e] - nb];
            V.dst_s[ep] = nmap[dst_s[eb + e] - nb];
        }
        base += __popcll(m);
    }
    if (lane == 0) erank[ne] = base;
    __syncthreads();
    // out slots: the old out_epos sequence restricted to kept edges, through the epos map
    base = 0;
    for (int c = 0; c < ne; c += WAVE) {
        const int j = c + lane;
        bool k = false;
        int ep = 0;
        if (j < ne) {
            const unsigned o = (unsigned)(out_epos[eb + j] - eb);
            if (o < (unsigned)ne) {
                ep = erank[o];
                k = erank[o + 1] > ep;
            }
        }
        const unsigned long long m = __ballot(k);
        const int r = base + lanes_below(m);
        if (j < ne) orank[j] = r;
        if (k) V.out_epos[eb2 + r] = eb2 + ep;
        base += __popcll(m);
    }
    if (lane == 0) orank[ne] = base;
    __syncthreads();
    // kept nodes: row pointers, and deg_rows (lane d counts this molecule's kept nodes of in-degree d so far)
    int seen = 0;
    for (int c = 0; c < n; c += WAVE) {
        const int i = c + lane;
        const int id = i < n ? nmap[i] : -1;
        int D = -1;
        if (id >= 0) {
            const int a = in_ptr[nb + i] - eb, b = in_ptr[nb + i + 1] - eb;
            V.in_ptr[id] = eb2 + erank[a];
            V.out_ptr[id] = eb2 + orank[out_ptr[nb + i] - eb];
            D = erank[b] - erank[a];
        }
        for (int d = 0; d < deg_stride; ++d) {
            const unsigned long long m = __ballot(D == d);
            if (m == 0) continue;
            const int before = __shfl(seen, d);
            if (D == d) {
                const int slot = V.deg_base[g * deg_stride + d] + before + lanes_below(m);
                if (slot >= 0 && slot < V.rows) V.deg_rows[slot] = id;
            }
            if (lane == d) seen += __popcll(m);
        }
    }
}

}  // namespace
}  // namespace i3d

using namespace i3d;

extern "C" int i3d_node_drop_build(const int64_t* src, const int64_t* dst, const int64_t* atom_feat, const int64_t* bond_feat,
                                   const int* in_ptr, const int* perm, const int* src_s, const int* dst_s, const int* out_ptr,
                                   const int* out_epos, const int* graph_ptr, int num_graphs, int atom_cols, int bond_cols,
                                   int max_atoms, int max_edges, int deg_stride, const I3dNodeDropView* views, int n_views,
                                   void* stream) {
    I3D_CHECK_ARG(num_graphs > 0 && atom_cols > 0 && bond_cols > 0 && max_atoms >= 0 && max_edges >= 0, "bad shape");
    I3D_CHECK_ARG(deg_stride >= 1 && deg_stride <= WAVE, "deg_stride: 1..64 (an in-degree per lane)");
    I3D_CHECK_ARG(views != nullptr && (n_views == 1 || n_views == 2), "n_views: 1 or 2");
    const long lds_bytes = (long)(max_atoms + 3 * max_edges + 2) * sizeof(int);
    I3D_CHECK_ARG(lds_bytes <= 65536, "molecule too large for one workgroup's LDS (max_atoms + 3 max_edges > 16382)");
    NodeDropViews v;
    v.v[0] = views[0];
    v.v[1] = views[n_views - 1];
    for (int k = 0; k < n_views; ++k)
        I3D_CHECK_ARG(views[k].keep && views[k].graph_ptr && views[k].edge_ptr && views[k].deg_base && views[k].num_nodes >= 0 &&
                          views[k].num_edges >= 0 && views[k].rows >= 0 && (views[k].n_groups == 0 || views[k].pad_range),
                      "view metadata");
    hipLaunchKernelGGL(node_drop_kernel, dim3(num_graphs, n_views), dim3(WAVE), lds_bytes, (hipStream_t)stream, src, dst,
                       atom_feat, bond_feat, in_ptr, perm, src_s, dst_s, out_ptr, out_epos, graph_ptr, atom_cols, bond_cols,
                       max_atoms, max_edges, deg_stride, v);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
