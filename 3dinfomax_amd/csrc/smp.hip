// SMP / SphereNet (reference models/spherical_message_passing.py, commons/spherical_encoding.py): the geometry and the two raw bases of
// a batch, once per batch, and the triplet interaction of update_e, once per layer and direction.  Forward only for the geometry:
// positions get no gradient (energy_and_force is refused by the module).
//
// Geometry.  Edges j -> i of the radius graph inside each molecule, no self loops, at most SMP_MAX_NBR in-neighbours per atom: the
// SMP_MAX_NBR lowest indices within range are kept (the scan of a molecule stops at the cap, as torch_cluster's device kernel stops
// at max_num_neighbors), so a capped graph may hold j -> i without i -> j.  The range test is fp32, d2 = (dx dx + dy dy) + dz dz <
// cutoff^2, the expression torch_cluster evaluates.  Edges are emitted sorted by destination i, sources ascending: the order the
// reference's SparseTensor(row = i, col = j) gives them.  Triplets k -> j -> i: for the edge e = (j -> i) every in-edge p = (k -> j)
// with k != i, in the order of p; idx_kj = p, idx_ji = e, grouped by e (trip_ptr).  Count launch, cumsum (the caller's), fill launch.
//
// Angle and torsion of a triplet are xyztodat's expressions, evaluated in fp64 from the fp32 positions and rounded once:
//   angle   = atan2(|ji x jk|, ji . jk)                                      ji = pos_i - pos_j, jk = pos_k - pos_j
//   torsion = min over the in-neighbours k_n != i of j of wrap(atan2((p1 x p2) . ji / |ji|, p1 . p2))   p1 = ji x jk, p2 = ji x (pos_kn - pos_j)
//   wrap(x) = x + 2 pi if x <= 0.  k_n == k: the two planes are the same vector, atan2(0, |p1|^2) = 0 -> exactly 2 pi; the value is
//   SET, not computed (a rounded cross product of a vector with itself need not vanish and a tiny positive result would win the minimum).
//
// Raw bases (no envelope, as the reference):  with x = zeros[l][q] dist_kj / cutoff and B[l][q] = norm[l][q] j_l(x),
//   sbf[t][l k + q]           = B[l][q] Y_l0(angle)                                         l < n, q < k
//   t[t][(f) k + q]           = B[f % n][q] Y_f(angle, torsion)                             f < n^2: the reference's pairing, kept
//   Y_f in the reference's list order: per l  [m = 0, cos m = 1..l, sin m = l..1], flat index l^2 + position;
//   Y_l0 = pref P_l0(cos a),  Y_lm = pref sin^m(a) {cos, sin}(m phi) P_lm(cos a), P_lm the polynomial part of the associated Legendre
//   function with the Condon-Shortley sign (P_mm = (1 - 2m) P_(m-1)(m-1)), pref the host's table (sqrt 2 folded in for m > 0).
// j_l in fp64: sin x / x for l = 0; the ascending series for x <= l (20 terms: the ratio of term m to the one before is x^2 / (2 m
// (2 l + 2 m + 1)) <= l^2 / (2 m (2 l + 2 m + 1)), at most 1.2 for the first term at l = 6 and below 0.6 from the second on, so the
// last term is below 1e-20 of the sum and the cancellation costs a digit at most); the upward recurrence from j_0, j_1 for x > l,
// where it is stable.  The closed forms the reference evaluates cancel badly at small x.
//
// Triplet interaction, out[e][c] = sum_{t in group e} x[idx_kj[t]][c] S_tc T_tc with S_tc = sum_b w1[c][b] s8[t][b], T_tc = sum_b
// w2[c][b] t8[t][b]:  no [T, I] tensor in either direction.
//   forward      wave = ji edge e; lane owns the columns lane + 64 r, r < R, with their rows of w1, w2 in registers.
//   backward 1   wave = ji edge e: per triplet the 2 Bs column sums ds8[t][b] = sum_c g x T w1[c][b], dt8[t][b] = sum_c g x S w2[c][b],
//                reduced across the wave by a halving butterfly (2 Bs values -> one per lane, then the remaining offsets).
//   backward 2   wave = kj edge p over the kj-grouped list (kj_ptr, kj_order): dx[p][c] = sum g[idx_ji[t]][c] S_tc T_tc, one writer per row.
//   backward 3,4 dw1, dw2 in fp64 over FIXED chunks of SMP_CHUNK triplets (thread = column), then per element over the chunks: four
//                waves, each a quarter of the chunks in chunk order, the four sums in wave order, rounded once.
// Every sum has a fixed order: no atomics, the same bits on every call.
// Lane map: int_emb <= 256 (R = 1, 2, 4), basis_emb <= 8 (padded to a power of two in registers); anything else is I3D_NOT_TAKEN.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): the widest shape taken, R = 4 at 8 basis columns, needs 224 per lane in the
// first backward pass and none in scratch; 16 basis columns would spill there (256 registers, 144 bytes of scratch per lane, one wave
// per SIMD) and no configuration of the reference uses more than 8, so the lane map stops at 8.
#include "common.h"

namespace i3d {

constexpr int SMP_MAX_NBR = 32;
constexpr int SMP_MAX_SPH = 7;
constexpr int SMP_MAX_RAD = 64;
constexpr int SMP_CHUNK = 256;
constexpr int SMP_FINAL_PARTS = 4;
constexpr int SMP_MAX_INT = 256;
constexpr int SMP_MAX_BASIS = 8;
constexpr double SMP_TWO_PI = 6.283185307179586476925286766559;

// ---- geometry ------------------------------------------------------------------------------------------------------------------
// thread = atom i: its in-neighbours, counted (src == nullptr) or written at in_ptr[i]
__global__ void __launch_bounds__(256)
smp_radius_kernel(const float* __restrict__ pos, const int* __restrict__ mol, const int* __restrict__ graph_ptr,
                  const int* __restrict__ in_ptr, int N, int B, int E, float r2, int* __restrict__ deg, int* __restrict__ src,
                  int* __restrict__ dst, float* __restrict__ dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int b = mol[i];
    int c = 0;
    if (b >= 0 && b < B) {
        const int beg = max(graph_ptr[b], 0), end = min(graph_ptr[b + 1], N);
        const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
        const int base = src ? in_ptr[i] : 0;
        for (int j = beg; j < end && c < SMP_MAX_NBR; ++j) {
            if (j == i) continue;
            const float dx = xi - pos[3 * j], dy = yi - pos[3 * j + 1], dz = zi - pos[3 * j + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < r2) {
                if (src && base + c >= 0 && base + c < E) {
                    src[base + c] = j;
                    dst[base + c] = i;
                    const double ex = (double)xi - (double)pos[3 * j], ey = (double)yi - (double)pos[3 * j + 1],
                                 ez = (double)zi - (double)pos[3 * j + 2];      // the distance in fp64 throughout; dx, dy, dz only decide
                    dist[base + c] = (float)sqrt((ex * ex + ey * ey) + ez * ez);
                }
                ++c;
            }
        }
    }
    if (!src) deg[i] = c;
}

// thread = edge e = (j -> i): its triplets (k -> j, k != i), counted (idx_kj == nullptr) or written at trip_ptr[e]
__global__ void __launch_bounds__(256)
smp_triplet_kernel(const int* __restrict__ src, const int* __restrict__ dst, const int* __restrict__ in_ptr,
                   const int* __restrict__ trip_ptr, int E, int T, int* __restrict__ count, int* __restrict__ idx_kj,
                   int* __restrict__ idx_ji) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int j = src[e], i = dst[e];
    const int beg = in_ptr[j], end = in_ptr[j + 1];
    int c = 0;
    const int base = idx_kj ? trip_ptr[e] : 0;
    for (int p = beg; p < end; ++p) {
        if (src[p] == i) continue;
        if (idx_kj && base + c >= 0 && base + c < T) {
            idx_kj[base + c] = p;
            idx_ji[base + c] = e;
        }
        ++c;
    }
    if (!idx_kj) count[e] = c;
}

__device__ __forceinline__ double smp_sph_jn(int l, double x) {
    if (l == 0) return x == 0. ? 1. : sin(x) / x;
    if (x <= (double)l) {
        double pre = 1.;
        for (int m = 1; m <= l; ++m) pre *= x / (double)(2 * m + 1);
        const double h = -0.5 * x * x;
        double term = 1., s = 1.;
        for (int m = 1; m <= 20; ++m) {
            term *= h / ((double)m * (double)(2 * l + 2 * m + 1));
            s += term;
        }
        return pre * s;
    }
    const double sx = sin(x), cx = cos(x);
    double jm = sx / x, jc = sx / (x * x) - cx / x;
    for (int m = 1; m < l; ++m) {
        const double jn = (double)(2 * m + 1) / x * jc - jm;
        jm = jc;
        jc = jn;
    }
    return jc;
}

// thread = (edge, l, q): the normalised Bessel value of the edge's distance
__global__ void __launch_bounds__(256)
smp_bessel_kernel(const float* __restrict__ dist, long total, int n, int k, double inv_cutoff, const double* __restrict__ zeros,
                  const double* __restrict__ norm, double* __restrict__ rbf) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int nk = n * k;
    const long e = idx / nk;
    const int r = (int)(idx % nk);
    const double x = zeros[r] * ((double)dist[e] * inv_cutoff);
    rbf[idx] = norm[r] * smp_sph_jn(r / k, x);
}

// thread = triplet: angle, torsion (fp32) and the n^2 real harmonics of (angle, torsion) in fp64
template <int NS>
__global__ void __launch_bounds__(256)
smp_angles_kernel(const float* __restrict__ pos, const int* __restrict__ src, const int* __restrict__ dst,
                  const int* __restrict__ in_ptr, const int* __restrict__ idx_kj, const int* __restrict__ idx_ji, int T,
                  const double* __restrict__ pref, float* __restrict__ angle, float* __restrict__ torsion, double* __restrict__ cbf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int e = idx_ji[t], p = idx_kj[t];
    const int i = dst[e], j = src[e], k = src[p];
    const double jx = pos[3 * j], jy = pos[3 * j + 1], jz = pos[3 * j + 2];
    const double ax = (double)pos[3 * i] - jx, ay = (double)pos[3 * i + 1] - jy, az = (double)pos[3 * i + 2] - jz;      // ji
    const double bx = (double)pos[3 * k] - jx, by = (double)pos[3 * k + 1] - jy, bz = (double)pos[3 * k + 2] - jz;      // jk
    const double dot = (ax * bx + ay * by) + az * bz;
    const double px = ay * bz - az * by, py = az * bx - ax * bz, pz = ax * by - ay * bx;                                // plane 1
    const double ang = atan2(sqrt((px * px + py * py) + pz * pz), dot);
    const double len = sqrt((ax * ax + ay * ay) + az * az);
    double tor = SMP_TWO_PI;                      // the candidate k_n == k, always present
    for (int q = in_ptr[j]; q < in_ptr[j + 1]; ++q) {
        const int kn = src[q];
        if (kn == i || kn == k) continue;
        const double cx = (double)pos[3 * kn] - jx, cy = (double)pos[3 * kn + 1] - jy, cz = (double)pos[3 * kn + 2] - jz;
        const double qx = ay * cz - az * cy, qy = az * cx - ax * cz, qz = ax * cy - ay * cx;                            // plane 2
        const double a = (px * qx + py * qy) + pz * qz;
        const double rx = py * qz - pz * qy, ry = pz * qx - px * qz, rz = px * qy - py * qx;
        const double b = ((rx * ax + ry * ay) + rz * az) / len;
        double cand = atan2(b, a);
        if (cand <= 0.) cand += SMP_TWO_PI;
        tor = fmin(tor, cand);
    }
    angle[t] = (float)ang;
    torsion[t] = (float)tor;
    // P[l][m], l < NS: polynomial parts of the associated Legendre functions at z = cos(angle)
    const double z = cos(ang), st = sin(ang);
    double P[NS][NS];
    P[0][0] = 1.;
#pragma unroll
    for (int m = 1; m < NS; ++m) P[m][m] = (double)(1 - 2 * m) * P[m - 1][m - 1];
#pragma unroll
    for (int m = 0; m < NS; ++m) {
        if (m + 1 < NS) P[m + 1][m] = (double)(2 * m + 1) * z * P[m][m];
#pragma unroll
        for (int l = m + 2; l < NS; ++l)
            P[l][m] = ((double)(2 * l - 1) * z * P[l - 1][m] - (double)(l + m - 1) * P[l - 2][m]) / (double)(l - m);
    }
    double cm[NS], sm[NS], sp[NS];      // cos(m phi), sin(m phi), sin^m(angle)
    cm[0] = 1., sm[0] = 0., sp[0] = 1.;
    const double c1 = cos(tor), s1 = sin(tor);
#pragma unroll
    for (int m = 1; m < NS; ++m) {
        cm[m] = cm[m - 1] * c1 - sm[m - 1] * s1;
        sm[m] = sm[m - 1] * c1 + cm[m - 1] * s1;
        sp[m] = sp[m - 1] * st;
    }
    double* row = cbf + (long)t * (NS * NS);
#pragma unroll
    for (int l = 0; l < NS; ++l) {
        const int f0 = l * l;
        row[f0] = pref[f0] * P[l][0];
#pragma unroll
        for (int m = 1; m <= l; ++m) {
            const double base = sp[m] * P[l][m];
            row[f0 + m] = pref[f0 + m] * (base * cm[m]);
            row[f0 + 2 * l + 1 - m] = pref[f0 + 2 * l + 1 - m] * (base * sm[m]);
        }
    }
}

// thread = one element of sbf, then of t
__global__ void __launch_bounds__(256)
smp_bases_kernel(const double* __restrict__ rbf, const double* __restrict__ cbf, const int* __restrict__ idx_kj, long T, int n, int k,
                 float* __restrict__ sbf, float* __restrict__ tb) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int nk = n * k, nn = n * n;
    const long nnk = (long)nn * k;
    const long first = T * nk;
    if (idx < first) {
        const long t = idx / nk;
        const int r = (int)(idx % nk), l = r / k;
        sbf[idx] = (float)(rbf[(long)idx_kj[t] * nk + r] * cbf[t * nn + l * l]);
    } else if (idx < first + T * nnk) {
        const long i2 = idx - first;
        const long t = i2 / nnk;
        const int r = (int)(i2 % nnk), f = r / k, q = r % k;
        tb[i2] = (float)(rbf[(long)idx_kj[t] * nk + (f % n) * k + q] * cbf[t * nn + f]);
    }
}

// ---- the triplet interaction -------------------------------------------------------------------------------------------------------
// NV values per lane -> lane L returns the wave's sum of value q(L) = sum_s bit_s(L) (NV >> (s + 1)), s < log2 NV
template <int NV>
__device__ __forceinline__ float smp_multi_reduce(float (&v)[NV], int lane) {
    int o = 1;
#pragma unroll
    for (int w = NV / 2; w >= 1; w >>= 1) {
        const bool hi = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < w; ++i) {
            const float send = hi ? v[i] : v[i + w];
            const float keep = hi ? v[i + w] : v[i];
            v[i] = keep + __shfl_xor(send, o);
        }
        o <<= 1;
    }
    for (; o < WAVE; o <<= 1) v[0] += __shfl_xor(v[0], o);
    return v[0];
}

template <int NV>
__device__ __forceinline__ int smp_reduce_slot(int lane) {
    int q = 0, s = 0;
#pragma unroll
    for (int w = NV / 2; w >= 1; w >>= 1, ++s) q += ((lane >> s) & 1) * w;
    return q;
}

template <int R, int BS>
struct SmpCols {
    float a1[R][BS], a2[R][BS];
    int col[R];
    bool live[R];
    __device__ __forceinline__ SmpCols(int lane, int I, int Bs, const float* __restrict__ w1, const float* __restrict__ w2) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            col[r] = lane + WAVE * r;
            live[r] = col[r] < I;
#pragma unroll
            for (int b = 0; b < BS; ++b) {
                const bool on = live[r] && b < Bs;
                a1[r][b] = on ? w1[(long)col[r] * Bs + b] : 0.f;
                a2[r][b] = on ? w2[(long)col[r] * Bs + b] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void products(int r, const float (&sv)[BS], const float (&tv)[BS], float& S, float& Tt) const {
        S = 0.f, Tt = 0.f;
#pragma unroll
        for (int b = 0; b < BS; ++b) {
            S += a1[r][b] * sv[b];
            Tt += a2[r][b] * tv[b];
        }
    }
};

template <int BS>
__device__ __forceinline__ void smp_load_basis(const float* __restrict__ s8, const float* __restrict__ t8, long t, int Bs, float (&sv)[BS],
                                               float (&tv)[BS]) {
#pragma unroll
    for (int b = 0; b < BS; ++b) {
        sv[b] = b < Bs ? s8[t * Bs + b] : 0.f;
        tv[b] = b < Bs ? t8[t * Bs + b] : 0.f;
    }
}

template <int R, int BS>
__global__ void __launch_bounds__(256)
smp_trip_fwd_kernel(const float* __restrict__ x, const float* __restrict__ s8, const float* __restrict__ t8, const float* __restrict__ w1,
                    const float* __restrict__ w2, const int* __restrict__ trip_ptr, const int* __restrict__ idx_kj, int E, int I, int Bs,
                    float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;                            // whole waves
    const int lane = threadIdx.x & 63;
    const SmpCols<R, BS> m(lane, I, Bs, w1, w2);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const int beg = trip_ptr[e], end = trip_ptr[e + 1];
#pragma unroll 2
    for (int t = beg; t < end; ++t) {
        const int kj = idx_kj[t];
        float sv[BS], tv[BS];
        smp_load_basis<BS>(s8, t8, t, Bs, sv, tv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!m.live[r]) continue;
            float S, Tt;
            m.products(r, sv, tv, S, Tt);
            acc[r] += x[(long)kj * I + m.col[r]] * S * Tt;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (m.live[r]) out[(long)e * I + m.col[r]] = acc[r];       // no triplets: an exact zero row
}

template <int R, int BS>
__global__ void __launch_bounds__(256)
smp_trip_bwd_ji_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ s8, const float* __restrict__ t8,
                       const float* __restrict__ w1, const float* __restrict__ w2, const int* __restrict__ trip_ptr,
                       const int* __restrict__ idx_kj, int E, int I, int Bs, float* __restrict__ ds8, float* __restrict__ dt8) {
    I3D_CHAIN_PRIO();
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const int lane = threadIdx.x & 63;
    const SmpCols<R, BS> m(lane, I, Bs, w1, w2);
    float gv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) gv[r] = m.live[r] ? g[(long)e * I + m.col[r]] : 0.f;
    const int slot = smp_reduce_slot<2 * BS>(lane);
    const int beg = trip_ptr[e], end = trip_ptr[e + 1];
    for (int t = beg; t < end; ++t) {
        const int kj = idx_kj[t];
        float sv[BS], tv[BS], v[2 * BS];
        smp_load_basis<BS>(s8, t8, t, Bs, sv, tv);
#pragma unroll
        for (int b = 0; b < 2 * BS; ++b) v[b] = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!m.live[r]) continue;
            float S, Tt;
            m.products(r, sv, tv, S, Tt);
            const float p = gv[r] * x[(long)kj * I + m.col[r]];
            const float dS = p * Tt, dT = p * S;
#pragma unroll
            for (int b = 0; b < BS; ++b) {
                v[b] += dS * m.a1[r][b];
                v[BS + b] += dT * m.a2[r][b];
            }
        }
        const float tot = smp_multi_reduce<2 * BS>(v, lane);
        if (lane < 2 * BS) {
            if (slot < BS) {
                if (slot < Bs) ds8[(long)t * Bs + slot] = tot;
            } else if (slot - BS < Bs) {
                dt8[(long)t * Bs + slot - BS] = tot;
            }
        }
    }
}

template <int R, int BS>
__global__ void __launch_bounds__(256)
smp_trip_bwd_kj_kernel(const float* __restrict__ g, const float* __restrict__ s8, const float* __restrict__ t8, const float* __restrict__ w1,
                       const float* __restrict__ w2, const int* __restrict__ kj_ptr, const int* __restrict__ kj_order,
                       const int* __restrict__ idx_ji, int E, int I, int Bs, float* __restrict__ dx) {
    I3D_CHAIN_PRIO();
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const int lane = threadIdx.x & 63;
    const SmpCols<R, BS> m(lane, I, Bs, w1, w2);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const int beg = kj_ptr[e], end = kj_ptr[e + 1];
#pragma unroll 2
    for (int p = beg; p < end; ++p) {
        const int t = kj_order[p];
        const int ji = idx_ji[t];
        float sv[BS], tv[BS];
        smp_load_basis<BS>(s8, t8, t, Bs, sv, tv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!m.live[r]) continue;
            float S, Tt;
            m.products(r, sv, tv, S, Tt);
            acc[r] += g[(long)ji * I + m.col[r]] * S * Tt;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (m.live[r]) dx[(long)e * I + m.col[r]] = acc[r];
}

// workgroup = chunk of SMP_CHUNK triplets, thread = column c: partial[chunk][0][c][b] (dw1), partial[chunk][1][c][b] (dw2) in fp64
template <int BS>
__global__ void __launch_bounds__(256)
smp_trip_bwd_w_chunk_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ s8,
                            const float* __restrict__ t8, const float* __restrict__ w1, const float* __restrict__ w2,
                            const int* __restrict__ idx_kj, const int* __restrict__ idx_ji, int T, int I, int Bs,
                            double* __restrict__ partial) {
    I3D_CHAIN_PRIO();
    const int c = threadIdx.x;
    if (c >= I) return;
    float a1[BS], a2[BS];
    double d1[BS], d2[BS];
#pragma unroll
    for (int b = 0; b < BS; ++b) {
        a1[b] = b < Bs ? w1[(long)c * Bs + b] : 0.f;
        a2[b] = b < Bs ? w2[(long)c * Bs + b] : 0.f;
        d1[b] = d2[b] = 0.;
    }
    const int t0 = blockIdx.x * SMP_CHUNK, t1 = min(t0 + SMP_CHUNK, T);
    for (int t = t0; t < t1; ++t) {
        float sv[BS], tv[BS];
        smp_load_basis<BS>(s8, t8, t, Bs, sv, tv);
        float S = 0.f, Tt = 0.f;
#pragma unroll
        for (int b = 0; b < BS; ++b) {
            S += a1[b] * sv[b];
            Tt += a2[b] * tv[b];
        }
        const float p = g[(long)idx_ji[t] * I + c] * x[(long)idx_kj[t] * I + c];
        const double dS = (double)(p * Tt), dT = (double)(p * S);
#pragma unroll
        for (int b = 0; b < BS; ++b) {
            d1[b] += dS * (double)sv[b];
            d2[b] += dT * (double)tv[b];
        }
    }
    double* row = partial + (long)blockIdx.x * 2 * I * Bs;
#pragma unroll
    for (int b = 0; b < BS; ++b)
        if (b < Bs) {
            row[(long)c * Bs + b] = d1[b];
            row[(long)I * Bs + (long)c * Bs + b] = d2[b];
        }
}

// workgroup = 64 elements of dw1 | dw2: wave w adds the w-th quarter of the chunks in chunk order, the four sums in wave order
__global__ void __launch_bounds__(256)
smp_trip_bwd_w_final_kernel(const double* __restrict__ partial, int chunks, int elems, float* __restrict__ dw1, float* __restrict__ dw2) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[SMP_FINAL_PARTS][WAVE];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int o = blockIdx.x * WAVE + lane;
    const int per = (chunks + SMP_FINAL_PARTS - 1) / SMP_FINAL_PARTS;
    const int lo = part * per, hi = min(lo + per, chunks);
    double s = 0.;
    if (o < 2 * elems) {
#pragma unroll 8
        for (int k = lo; k < hi; ++k) s += partial[(long)k * 2 * elems + o];
    }
    sm[part][lane] = s;
    __syncthreads();
    if (part == 0 && o < 2 * elems) {
        const float v = (float)(((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane]);
        if (o < elems) dw1[o] = v;
        else dw2[o - elems] = v;
    }
}

struct SmpPlan {
    int R, BS;
};

static int smp_plan(const char* who, int int_emb, int basis_emb, SmpPlan* p) {
    if (int_emb < 1 || basis_emb < 1) {
        set_error("%s: invalid argument: int_emb / basis_emb below 1", who);
        return I3D_ERR_INVALID;
    }
    if (int_emb > SMP_MAX_INT || basis_emb > SMP_MAX_BASIS) return I3D_NOT_TAKEN;
    p->R = int_emb <= 64 ? 1 : (int_emb <= 128 ? 2 : 4);
    p->BS = 1;
    while (p->BS < basis_emb) p->BS <<= 1;
    return I3D_OK;
}

}  // namespace i3d

using namespace i3d;

#define SMP_DISPATCH_BS(KERNEL, RR, ...)                                                                                           \
    do {                                                                                                                           \
        if (plan.BS == 1) hipLaunchKernelGGL((KERNEL<RR, 1>), grid_, dim3(256), 0, s_, __VA_ARGS__);                               \
        else if (plan.BS == 2) hipLaunchKernelGGL((KERNEL<RR, 2>), grid_, dim3(256), 0, s_, __VA_ARGS__);                          \
        else if (plan.BS == 4) hipLaunchKernelGGL((KERNEL<RR, 4>), grid_, dim3(256), 0, s_, __VA_ARGS__);                          \
        else hipLaunchKernelGGL((KERNEL<RR, 8>), grid_, dim3(256), 0, s_, __VA_ARGS__);                                            \
    } while (0)

#define SMP_DISPATCH(KERNEL, ...)                                                                                                  \
    do {                                                                                                                           \
        const dim3 grid_(cdiv(num_edges, 4));                                                                                      \
        hipStream_t s_ = (hipStream_t)stream;                                                                                      \
        if (plan.R == 1) SMP_DISPATCH_BS(KERNEL, 1, __VA_ARGS__);                                                                  \
        else if (plan.R == 2) SMP_DISPATCH_BS(KERNEL, 2, __VA_ARGS__);                                                             \
        else SMP_DISPATCH_BS(KERNEL, 4, __VA_ARGS__);                                                                              \
    } while (0)

extern "C" int i3d_smp_max_neighbors(void) { return SMP_MAX_NBR; }

extern "C" int i3d_smp_radius_count(const float* pos, const int* mol, const int* graph_ptr, int num_nodes, int num_graphs, float cutoff,
                                    int* deg, void* stream) {
    I3D_CHECK_ARG(num_nodes >= 0 && num_graphs >= 0 && cutoff > 0.f, "num_nodes / num_graphs below 0 or cutoff not positive");
    if (num_nodes == 0) return I3D_OK;
    I3D_CHECK_ARG(pos && mol && graph_ptr && deg, "null pointer");
    hipLaunchKernelGGL(smp_radius_kernel, dim3(cdiv(num_nodes, 256)), dim3(256), 0, (hipStream_t)stream, pos, mol, graph_ptr,
                       (const int*)nullptr, num_nodes, num_graphs, 0, cutoff * cutoff, deg, (int*)nullptr, (int*)nullptr, (float*)nullptr);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_radius_fill(const float* pos, const int* mol, const int* graph_ptr, const int* in_ptr, int num_nodes,
                                   int num_graphs, int num_edges, float cutoff, int* src, int* dst, float* dist, void* stream) {
    I3D_CHECK_ARG(num_nodes >= 0 && num_graphs >= 0 && num_edges >= 0 && cutoff > 0.f,
                  "num_nodes / num_graphs / num_edges below 0 or cutoff not positive");
    if (num_nodes == 0 || num_edges == 0) return I3D_OK;
    I3D_CHECK_ARG(pos && mol && graph_ptr && in_ptr && src && dst && dist, "null pointer");
    hipLaunchKernelGGL(smp_radius_kernel, dim3(cdiv(num_nodes, 256)), dim3(256), 0, (hipStream_t)stream, pos, mol, graph_ptr, in_ptr,
                       num_nodes, num_graphs, num_edges, cutoff * cutoff, (int*)nullptr, src, dst, dist);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_triplet_count(const int* src, const int* dst, const int* in_ptr, int num_edges, int* count, void* stream) {
    I3D_CHECK_ARG(num_edges >= 0, "num_edges below 0");
    if (num_edges == 0) return I3D_OK;
    I3D_CHECK_ARG(src && dst && in_ptr && count, "null pointer");
    hipLaunchKernelGGL(smp_triplet_kernel, dim3(cdiv(num_edges, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, in_ptr,
                       (const int*)nullptr, num_edges, 0, count, (int*)nullptr, (int*)nullptr);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_triplet_fill(const int* src, const int* dst, const int* in_ptr, const int* trip_ptr, int num_edges,
                                    int num_triplets, int* idx_kj, int* idx_ji, void* stream) {
    I3D_CHECK_ARG(num_edges >= 0 && num_triplets >= 0, "num_edges / num_triplets below 0");
    if (num_edges == 0 || num_triplets == 0) return I3D_OK;
    I3D_CHECK_ARG(src && dst && in_ptr && trip_ptr && idx_kj && idx_ji, "null pointer");
    hipLaunchKernelGGL(smp_triplet_kernel, dim3(cdiv(num_edges, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, in_ptr, trip_ptr,
                       num_edges, num_triplets, (int*)nullptr, idx_kj, idx_ji);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_bases(const float* pos, const float* dist, const int* src, const int* dst, const int* in_ptr, const int* idx_kj,
                             const int* idx_ji, int num_edges, int num_triplets, int num_spherical, int num_radial, float cutoff,
                             const double* zeros, const double* norm, const double* pref, double* rbf_ws, double* cbf_ws, float* angle,
                             float* torsion, float* sbf, float* t, void* stream) {
    I3D_CHECK_ARG(num_edges >= 0 && num_triplets >= 0 && cutoff > 0.f, "num_edges / num_triplets below 0 or cutoff not positive");
    I3D_CHECK_ARG(num_spherical >= 1 && num_spherical <= SMP_MAX_SPH && num_radial >= 1 && num_radial <= SMP_MAX_RAD,
                  "num_spherical outside 1..7 or num_radial outside 1..64");
    if (num_edges == 0 || num_triplets == 0) return I3D_OK;
    I3D_CHECK_ARG(pos && dist && src && dst && in_ptr && idx_kj && idx_ji && zeros && norm && pref && rbf_ws && cbf_ws && angle &&
                      torsion && sbf && t, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int n = num_spherical, k = num_radial;
    const long nrbf = (long)num_edges * n * k;
    hipLaunchKernelGGL(smp_bessel_kernel, dim3(cdiv(nrbf, 256)), dim3(256), 0, s, dist, nrbf, n, k, 1. / (double)cutoff, zeros, norm, rbf_ws);
    I3D_CHECK_LAUNCH();
    const dim3 tg(cdiv(num_triplets, 256));
#define SMP_ANGLES(NS)                                                                                                             \
    case NS:                                                                                                                       \
        hipLaunchKernelGGL(smp_angles_kernel<NS>, tg, dim3(256), 0, s, pos, src, dst, in_ptr, idx_kj, idx_ji, num_triplets, pref, angle, \
                           torsion, cbf_ws);                                                                                       \
        break
    switch (n) {
        SMP_ANGLES(1);
        SMP_ANGLES(2);
        SMP_ANGLES(3);
        SMP_ANGLES(4);
        SMP_ANGLES(5);
        SMP_ANGLES(6);
        SMP_ANGLES(7);
    }
#undef SMP_ANGLES
    I3D_CHECK_LAUNCH();
    const long total = (long)num_triplets * ((long)n * k + (long)n * n * k);
    hipLaunchKernelGGL(smp_bases_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, (const double*)rbf_ws, (const double*)cbf_ws, idx_kj,
                       (long)num_triplets, n, k, sbf, t);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_triplets_takes(int int_emb, int basis_emb) {
    SmpPlan plan;
    return smp_plan("i3d_smp_triplets_takes", int_emb, basis_emb, &plan);
}

extern "C" int i3d_smp_triplets_chunk(void) { return SMP_CHUNK; }

extern "C" long i3d_smp_triplets_bwd_partial_floats(int num_triplets, int int_emb, int basis_emb) {
    if (num_triplets < 0 || int_emb < 1 || basis_emb < 1) return 0;
    const long chunks = ((long)num_triplets + SMP_CHUNK - 1) / SMP_CHUNK;
    return 2L * chunks * 2L * int_emb * basis_emb;        // fp64
}

extern "C" int i3d_smp_triplets_fwd(const float* x, const float* s8, const float* t8, const float* w1, const float* w2,
                                    const int* trip_ptr, const int* idx_kj, int num_edges, int num_triplets, int int_emb, int basis_emb,
                                    float* out, void* stream) {
    SmpPlan plan;
    if (int rc = smp_plan(__func__, int_emb, basis_emb, &plan)) return rc;
    I3D_CHECK_ARG(num_edges >= 0 && num_triplets >= 0, "num_edges / num_triplets below 0");
    if (num_edges == 0) return I3D_OK;
    I3D_CHECK_ARG(x && w1 && w2 && trip_ptr && out, "null pointer");
    I3D_CHECK_ARG(num_triplets == 0 || (s8 && t8 && idx_kj), "triplets without s8 / t8 / idx_kj");
    SMP_DISPATCH(smp_trip_fwd_kernel, x, s8, t8, w1, w2, trip_ptr, idx_kj, num_edges, int_emb, basis_emb, out);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_smp_triplets_bwd(const float* g, const float* x, const float* s8, const float* t8, const float* w1, const float* w2,
                                    const int* trip_ptr, const int* idx_kj, const int* idx_ji, const int* kj_ptr, const int* kj_order,
                                    int num_edges, int num_triplets, int int_emb, int basis_emb, float* partials, float* dx, float* ds8,
                                    float* dt8, float* dw1, float* dw2, void* stream) {
    SmpPlan plan;
    if (int rc = smp_plan(__func__, int_emb, basis_emb, &plan)) return rc;
    I3D_CHECK_ARG(num_edges >= 1 && num_triplets >= 1, "num_edges / num_triplets below 1 (the caller returns zeros)");
    I3D_CHECK_ARG(g && x && s8 && t8 && w1 && w2 && trip_ptr && idx_kj && idx_ji && kj_ptr && kj_order && partials && dx && ds8 && dt8 &&
                      dw1 && dw2, "null pointer");
    I3D_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "partials not 8-byte aligned");
    SMP_DISPATCH(smp_trip_bwd_ji_kernel, g, x, s8, t8, w1, w2, trip_ptr, idx_kj, num_edges, int_emb, basis_emb, ds8, dt8);
    I3D_CHECK_LAUNCH();
    SMP_DISPATCH(smp_trip_bwd_kj_kernel, g, s8, t8, w1, w2, kj_ptr, kj_order, idx_ji, num_edges, int_emb, basis_emb, dx);
    I3D_CHECK_LAUNCH();
    const int chunks = cdiv(num_triplets, SMP_CHUNK);
    double* part = reinterpret_cast<double*>(partials);
    const dim3 cgrid(chunks), cblock(cdiv(int_emb, WAVE) * WAVE);
    hipStream_t s = (hipStream_t)stream;
#define SMP_CHUNK_LAUNCH(BB)                                                                                                       \
    case BB:                                                                                                                       \
        hipLaunchKernelGGL(smp_trip_bwd_w_chunk_kernel<BB>, cgrid, cblock, 0, s, g, x, s8, t8, w1, w2, idx_kj, idx_ji, num_triplets,  \
                           int_emb, basis_emb, part);                                                                              \
        break
    switch (plan.BS) {
        SMP_CHUNK_LAUNCH(1);
        SMP_CHUNK_LAUNCH(2);
        SMP_CHUNK_LAUNCH(4);
        SMP_CHUNK_LAUNCH(8);
    }
#undef SMP_CHUNK_LAUNCH
    I3D_CHECK_LAUNCH();
    const int elems = int_emb * basis_emb;
    hipLaunchKernelGGL(smp_trip_bwd_w_final_kernel, dim3(cdiv(2 * elems, WAVE)), dim3(256), 0, s, (const double*)part, chunks, elems, dw1,
                       dw2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
