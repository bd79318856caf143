// Set-matching and per-conformer NT-Xent losses of the multi-conformer ablations: NTXentMinimumMatching (reference commons/losses.py:
// 747-794), NTXentMaximumSimilarity (:839-886), NTXentMultiplePositivesV2 (:598-643) and NTXentMultiplePositivesV3 (:646-689).
// B molecules, C conformers, D features, s' = S / (|z1 row| |z2 row|) (the norms are ones without normalisation), P = exp(s' / tau).
// No epsilon anywhere; a zero row gives NaN as in the reference.
//
//   matching     z1v [N, D] (N = B C, one 2D embedding per conformer), z2 [N, D]; S [N, N] = z1v z2^T comes from the GEMM, rows (i, l),
//                columns (j, u).  pair: one wave per molecule pair (i, j), lane l C + u holds s'[(i, l), (j, u)] (C <= 8: at most 64
//                lanes); a butterfly over (value, lane) gives the lane of the block minimum (min mode: plus the conformer l of the
//                largest matched entry l == u) or of the block maximum (max mode).  exp is monotone: the selection is made on s' and
//                only the selected entries are ever exponentiated.  The tables [B, B] hold one byte per pair, the lane; the value is
//                read again from S in fp64 wherever it is needed (an fp32 copy of s' would add its rounding times 1 / tau).
//                row: one workgroup per molecule i: den_i = sum_{j != i} exp(sel_ij / tau) over the off-diagonal pairs themselves (no
//                sum - diagonal), in fp64 and in a fixed order; the positive is exp(max_ii / tau) (max mode) or, in min mode, the
//                largest MATCHED entry s'[(i, l), (j, l)] over EVERY column molecule j and every l - the reference's torch.amax(torch.
//                diagonal(sim, dim1=2, dim2=3), dim=(1, 2)) runs over j too, not only over j = i.  Its place (j*, l*) is recorded.
//                backward: one selected entry (r, c) per molecule pair with weight W = dL/ds' = g / (B den_i) exp(sel_ij / tau) / tau,
//                and one entry per molecule for the positive with W = -g / (B tau) (at C = 1 it can be a negative's entry too: the
//                two add).  d s'/d z1_r = z2_c / (a_r b_c) - s' z1_r / a_r^2, and likewise for z2_c.  A weight pass writes the
//                coefficients per pair ([i][j] order and transposed), then two gather kernels: for dz1 one workgroup per row molecule
//                i walks j = 0 .. B - 1 in order, for dz2 one per column molecule j walks i in order; a thread owns one feature and
//                keeps the molecule's C rows in registers.  No dense dL/dS, no backward GEMM, no atomics.
//   tie rule     the lowest lane (l, then u) wins a tie inside a block, the lowest j (then the lowest l) a tie between the candidates
//                of the positive.  torch splits the gradient of a tie evenly between the tied entries; a tie has measure zero.  A NaN
//                wins every selection, so it reaches the loss as it does through torch.amin / torch.amax.
//   per conf.    z1 [B, D], z2 [N, D] molecule major, S [B, N] = z1 z2^T.  V2: pos_i = sum_u P[i, (i, u)], den_i = sum_{j != i}
//                P[i, (j, 0)] - only conformer 0 of the other molecules is a negative -, loss = -mean_i log(pos_i / den_i).  V3: for
//                every (i, u): pos = P[i, (i, u)], den = sum_{j != i} P[i, (j, u)], loss = -mean over the B C pairs.  forward: one
//                workgroup per row; a thread keeps its conformer (the stride over the columns is the largest multiple of C that fits
//                the workgroup), the positives are left out of the sums, never subtracted; fp64, fixed order.  backward: a row pass
//                writes dS [B, N] (exact zeros in V2's unused columns) and the rows' norm coefficient, a column pass the columns'.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace i3d {

constexpr int CM_MAX_CONF = 8;           // C^2 lanes of one wave
constexpr int PC_MAX_CONF = 64;          // every conformer keeps at least four threads of the row kernel
constexpr int CM_MIN = 0, CM_MAX = 1;
constexpr int CM_GATHER_U = 8;          // rows in flight per thread of the gather kernels
constexpr int PC_V2 = 0, PC_V3 = 1;

// does the candidate (ov, oi) replace (v, i)?  A strict total order on pairs with distinct indices, so a butterfly leaves the same
// winner in every lane
template <bool MAXSEL>
__device__ __forceinline__ bool cm_takes(double ov, int oi, double v, int i) {
    const bool on = ov != ov, vn = v != v;
    if (on || vn) return on && (!vn || oi < i);
    if (ov == v) return oi < i;
    return MAXSEL ? ov > v : ov < v;
}

template <bool MAXSEL>
__device__ __forceinline__ void cm_wave_select(double& v, int& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (cm_takes<MAXSEL>(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ double cm_sprime(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
                                            long N, long r, long c) {
    return (double)sim[r * N + c] / ((double)n1[r] * (double)n2[c]);
}

// ---- matching: selection --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cm_pair_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2, int B, int C, int mode,
               unsigned char* __restrict__ sel, unsigned char* __restrict__ dsel) {
    I3D_CHAIN_PRIO();
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long)B * B) return;          // the whole wave
    const int i = (int)(pair / B), j = (int)(pair - (long)i * B);
    const int CC = C * C;
    const long N = (long)B * C;
    const bool on = lane < CC;
    const int l = on ? lane / C : 0, u = on ? lane - l * C : 0;          // the other lanes read entry (0, 0) of the block
    const double s = cm_sprime(sim, n1, n2, N, (long)i * C + l, (long)j * C + u);
    if (mode == CM_MIN) {
        double v = on ? s : (double)INFINITY;
        int k = lane;
        cm_wave_select<false>(v, k);
        double dv = (on && l == u) ? s : -(double)INFINITY;
        int dk = lane;
        cm_wave_select<true>(dv, dk);
        if (lane == 0) {
            sel[pair] = (unsigned char)(k < CC ? k : 0);
            dsel[pair] = (unsigned char)(dk < CC ? dk / C : 0);
        }
    } else {
        double v = on ? s : -(double)INFINITY;
        int k = lane;
        cm_wave_select<true>(v, k);
        if (lane == 0) sel[pair] = (unsigned char)(k < CC ? k : 0);
    }
}

// ---- matching: per-molecule sums ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cm_row_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2, int B, int C, int mode,
              double inv_tau, const unsigned char* __restrict__ sel, const unsigned char* __restrict__ dsel,
              double* __restrict__ row_den, double* __restrict__ row_pos, int* __restrict__ pos_j, int* __restrict__ pos_lu) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    __shared__ double bv[4];
    __shared__ int bj[4], bq[4];
    const int i = blockIdx.x;
    const int CC = C * C;
    const long N = (long)B * C;
    double den = 0., best = -(double)INFINITY;
    int jb = INT_MAX, qb = 0;
    for (int j = threadIdx.x; j < B; j += 256) {
        int q = sel[(long)i * B + j];
        if (q >= CC) q = 0;
        const int l = q / C, u = q - l * C;
        const double s = cm_sprime(sim, n1, n2, N, (long)i * C + l, (long)j * C + u);
        if (j != i) den += exp(s * inv_tau);
        if (mode == CM_MIN) {
            int d = dsel[(long)i * B + j];
            if (d >= C) d = 0;
            const double sd = cm_sprime(sim, n1, n2, N, (long)i * C + d, (long)j * C + d);
            if (cm_takes<true>(sd, j, best, jb)) {
                best = sd;
                jb = j;
                qb = d * C + d;
            }
        } else if (j == i) {
            best = s;
            jb = j;
            qb = q;
        }
    }
    den = block_sum_f64(den, sm);
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const int oj = __shfl_xor(jb, o), oq = __shfl_xor(qb, o);
        if (cm_takes<true>(ov, oj, best, jb)) {
            best = ov;
            jb = oj;
            qb = oq;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        bv[w] = best;
        bj[w] = jb;
        bq[w] = qb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k)
            if (cm_takes<true>(bv[k], bj[k], best, jb)) {
                best = bv[k];
                jb = bj[k];
                qb = bq[k];
            }
        row_den[i] = den;
        row_pos[i] = exp(best * inv_tau);
        pos_j[i] = (jb >= 0 && jb < B) ? jb : i;
        pos_lu[i] = (qb >= 0 && qb < CC) ? qb : 0;
    }
}

// loss = -mean over `count` entries of log(pos / den), in order
__global__ void __launch_bounds__(256)
cm_loss_kernel(const double* __restrict__ den, const double* __restrict__ pos, int count, float* __restrict__ loss) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    double acc = 0.;
    for (int i = threadIdx.x; i < count; i += 256) acc -= log(pos[i] / den[i]);
    acc = block_sum_f64(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(acc / (double)count);
}

// ---- matching: backward ---------------------------------------------------------------------------------------------------------
// one thread per molecule pair: the coefficients of its selected entry (r, c), W = dL/ds':  wz = W / (a_r b_c) (times z2_c into dz1_r,
// times z1_r into dz2_c), wsa = -W s' / a_r^2 (times z1_r into dz1_r), wsb = -W s' / b_c^2 (times z2_c into dz2_c); the last two and
// the lane also in [j][i] order for the column pass.  The diagonal pair carries no negative; its thread writes the coefficients of the
// molecule's positive instead.
__global__ void __launch_bounds__(256)
cm_weight_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
                 const unsigned char* __restrict__ sel, const double* __restrict__ row_den, const int* __restrict__ pos_j,
                 const int* __restrict__ pos_lu, int B, int C, int norm, double inv_tau, const float* __restrict__ gs_dev,
                 float* __restrict__ wz, float* __restrict__ wsa, float* __restrict__ wzT, float* __restrict__ wsbT,
                 unsigned char* __restrict__ selT, float* __restrict__ pwz, float* __restrict__ pwsa, float* __restrict__ pwsb) {
    I3D_CHAIN_PRIO();
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * B) return;
    const int i = (int)(t / B), j = (int)(t - (long)i * B);
    const int CC = C * C;
    const long N = (long)B * C;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / (double)B;
    int q = sel[t];
    if (q >= CC) q = 0;
    float z = 0.f, sa = 0.f, sb = 0.f;
    if (j != i) {
        const int l = q / C, u = q - l * C;
        const long r = (long)i * C + l, c = (long)j * C + u;
        const double a = (double)n1[r], b = (double)n2[c];
        const double s = (double)sim[r * N + c] / (a * b);
        const double W = gs / row_den[i] * exp(s * inv_tau) * inv_tau;
        z = (float)(W / (a * b));
        if (norm) {
            sa = (float)(-W * s / (a * a));
            sb = (float)(-W * s / (b * b));
        }
    } else {
        int jj = pos_j[i], p = pos_lu[i];
        if (jj < 0 || jj >= B) jj = i;
        if (p < 0 || p >= CC) p = 0;
        const int l = p / C, u = p - l * C;
        const long r = (long)i * C + l, c = (long)jj * C + u;
        const double a = (double)n1[r], b = (double)n2[c];
        const double s = (double)sim[r * N + c] / (a * b);
        const double W = -gs * inv_tau;
        pwz[i] = (float)(W / (a * b));
        pwsa[i] = norm ? (float)(-W * s / (a * a)) : 0.f;
        pwsb[i] = norm ? (float)(-W * s / (b * b)) : 0.f;
    }
    const long tt = (long)j * B + i;
    wz[t] = z;
    wsa[t] = sa;
    wzT[tt] = z;
    wsbT[tt] = sb;
    selT[tt] = (unsigned char)q;
}

// out[(m, k), d] = sum over the partner molecules p, in order, of w[m, p] other[(p, ot), d] [k == lo] + (sum of ws[m, p] [k == lo])
// own[(m, k), d], plus the positives.  ROWS: m = i, the partners are the column molecules, own = z1v, other = z2, the tables in
// [i][j] order, and the molecule's own positive is added last.  !ROWS: m = j, the partners are the row molecules, own = z2,
// other = z1v, the tables in [j][i] order, and the positive of every row molecule whose j* is m is added at its turn.  One feature
// per thread (blockIdx.y: chunks of 256 features); the partners' coefficients go through LDS 256 at a time.
template <bool ROWS>
__global__ void __launch_bounds__(256)
cm_gather_kernel(const float* __restrict__ own, const float* __restrict__ other, const float* __restrict__ w,
                 const float* __restrict__ ws, const unsigned char* __restrict__ lu, const int* __restrict__ pos_j,
                 const int* __restrict__ pos_lu, const float* __restrict__ pwz, const float* __restrict__ pws, int B, int C, int D,
                 float* __restrict__ out) {
    I3D_CHAIN_PRIO();
    __shared__ float s_w[256], s_s[256], s_pw[256], s_ps[256];
    __shared__ unsigned char s_lo[256], s_ot[256], s_plo[256], s_pot[256];
    const int m = blockIdx.x;
    const int d = blockIdx.y * 256 + threadIdx.x;
    const bool dok = d < D;
    const int CC = C * C;
    double acc[CM_MAX_CONF], self[CM_MAX_CONF];
#pragma unroll
    for (int k = 0; k < CM_MAX_CONF; ++k) acc[k] = self[k] = 0.;
    for (int p0 = 0; p0 < B; p0 += 256) {
        __syncthreads();
        const int p = p0 + threadIdx.x;
        if (p < B) {
            const long e = (long)m * B + p;
            int q = lu[e];
            if (q >= CC) q = 0;
            const int l = q / C, u = q - l * C;
            s_lo[threadIdx.x] = (unsigned char)(ROWS ? l : u);
            s_ot[threadIdx.x] = (unsigned char)(ROWS ? u : l);
            s_w[threadIdx.x] = w[e];
            s_s[threadIdx.x] = ws[e];
            if (!ROWS) {
                unsigned char plo = 255, pot = 0;
                float pw = 0.f, ps = 0.f;
                if (pos_j[p] == m) {
                    int q2 = pos_lu[p];
                    if (q2 < 0 || q2 >= CC) q2 = 0;
                    pot = (unsigned char)(q2 / C);
                    plo = (unsigned char)(q2 - (q2 / C) * C);
                    pw = pwz[p];
                    ps = pws[p];
                }
                s_plo[threadIdx.x] = plo;
                s_pot[threadIdx.x] = pot;
                s_pw[threadIdx.x] = pw;
                s_ps[threadIdx.x] = ps;
            }
        }
        __syncthreads();
        const int n = B - p0 < 256 ? B - p0 : 256;
        // CM_GATHER_U partners at a time: their rows are requested together (the row's address comes out of LDS, so one partner at
        // a time would pay a full memory latency each), then added in order
        for (int t0 = 0; t0 < n; t0 += CM_GATHER_U) {
            float x[CM_GATHER_U];
#pragma unroll
            for (int q = 0; q < CM_GATHER_U; ++q) {
                const int t = t0 + q;
                x[q] = (dok && t < n) ? other[((long)(p0 + t) * C + s_ot[t]) * D + d] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < CM_GATHER_U; ++q) {
                const int t = t0 + q;
                const bool ok = t < n;
                const int lo = s_lo[t];
                const double wx = ok ? (double)s_w[t] * (double)x[q] : 0., sv = ok ? (double)s_s[t] : 0.;
#pragma unroll
                for (int k = 0; k < CM_MAX_CONF; ++k) {
                    acc[k] += k == lo ? wx : 0.;
                    self[k] += k == lo ? sv : 0.;
                }
                if (!ROWS && ok && s_plo[t] != 255) {          // the same for every thread of the workgroup
                    const int plo = s_plo[t];
                    const float px = dok ? other[((long)(p0 + t) * C + s_pot[t]) * D + d] : 0.f;
                    const double pwx = (double)s_pw[t] * (double)px, psv = (double)s_ps[t];
#pragma unroll
                    for (int k = 0; k < CM_MAX_CONF; ++k) {
                        acc[k] += k == plo ? pwx : 0.;
                        self[k] += k == plo ? psv : 0.;
                    }
                }
            }
        }
    }
    if (ROWS) {
        int jj = pos_j[m], q2 = pos_lu[m];
        if (jj < 0 || jj >= B) jj = m;
        if (q2 < 0 || q2 >= CC) q2 = 0;
        const int plo = q2 / C, pot = q2 - plo * C;
        const float px = dok ? other[((long)jj * C + pot) * D + d] : 0.f;
        const double pwx = (double)pwz[m] * (double)px, psv = (double)pws[m];
#pragma unroll
        for (int k = 0; k < CM_MAX_CONF; ++k) {
            acc[k] += k == plo ? pwx : 0.;
            self[k] += k == plo ? psv : 0.;
        }
    }
    if (!dok) return;
#pragma unroll
    for (int k = 0; k < CM_MAX_CONF; ++k) {
        if (k >= C) break;
        const long r = (long)m * C + k;
        out[r * D + d] = (float)(acc[k] + self[k] * (double)own[r * D + d]);
    }
}

// ---- per-conformer losses -------------------------------------------------------------------------------------------------------
// one workgroup per row i of S [B, N]; thread t < stride = (256 / C) C reads the columns t, t + stride, ...: all of conformer t % C
template <bool V3>
__global__ void __launch_bounds__(256)
pc_fwd_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2, int B, int C, double inv_tau,
              double* __restrict__ den, double* __restrict__ pos) {
    I3D_CHAIN_PRIO();
    __shared__ double sd[256], sp[256];
    const int i = blockIdx.x, t = threadIdx.x;
    const long N = (long)B * C;
    const int stride = (256 / C) * C;
    double den_t = 0., pos_t = 0.;
    if (t < stride) {
        const int u = t % C;
        const double a = (double)n1[i];
        for (long c = t; c < N; c += stride) {
            const bool own = c / C == i;
            if (!V3 && !own && u != 0) continue;          // V2: conformer 0 is the only negative
            const double p = exp((double)sim[(long)i * N + c] / (a * (double)n2[c]) * inv_tau);
            if (own) pos_t += p;
            else den_t += p;
        }
    }
    sd[t] = den_t;
    sp[t] = pos_t;
    __syncthreads();
    if (V3) {
        if (t < C) {
            double dsum = 0., psum = 0.;
            for (int k = t; k < stride; k += C) {
                dsum += sd[k];
                psum += sp[k];
            }
            den[(long)i * C + t] = dsum;
            pos[(long)i * C + t] = psum;
        }
    } else if (t == 0) {
        double dsum = 0., psum = 0.;
        for (int k = 0; k < stride; k += C) dsum += sd[k];
        for (int k = 0; k < stride; ++k) psum += sp[k];
        den[i] = dsum;
        pos[i] = psum;
    }
}

// dS = H = dL/dP P / tau / (a b);  dL/dP = -g / (M pos) at a positive, g / (M den) at a negative (M = B, or B C terms in V3), 0 elsewhere;
// ca_i = -(1 / a_i) sum_c H s' b_c
template <bool V3>
__global__ void __launch_bounds__(256)
pc_bwd_row_kernel(const float* __restrict__ sim, const float* __restrict__ n1, const float* __restrict__ n2,
                  const double* __restrict__ den, const double* __restrict__ pos, int B, int C, double inv_tau,
                  const float* __restrict__ gs_dev, float* __restrict__ dsim, float* __restrict__ ca) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[4];
    const int i = blockIdx.x;
    const long N = (long)B * C;
    const double gs = (gs_dev ? (double)gs_dev[0] : 1.) / (V3 ? (double)B * (double)C : (double)B);
    const double a = (double)n1[i];
    double da = 0.;
    for (long c = threadIdx.x; c < N; c += 256) {
        const long j = c / C;
        const int u = (int)(c - j * C);
        const bool own = j == i;
        float h = 0.f;
        if (own || V3 || u == 0) {
            const double b = (double)n2[c], nrm = a * b;
            const double s = (double)sim[(long)i * N + c] / nrm;
            const long k = V3 ? (long)i * C + u : i;
            const double H = (own ? -gs / pos[k] : gs / den[k]) * exp(s * inv_tau) * inv_tau / nrm;
            h = (float)H;
            da -= H * s * b;
        }
        dsim[(long)i * N + c] = h;
    }
    da = block_sum_f64(da, sm);
    if (threadIdx.x == 0) ca[i] = a > 0. ? (float)(da / a) : 0.f;
}

// cb_c = -(1 / b_c) sum_r H[r, c] s'[r, c] a_r over the B rows: 16 columns per workgroup, 16 row lanes, their partials summed in order
constexpr int PC_COL_W = 16, PC_COL_L = 16;
__global__ void __launch_bounds__(256)
pc_bwd_col_kernel(const float* __restrict__ sim, const float* __restrict__ dsim, const float* __restrict__ n1,
                  const float* __restrict__ n2, int B, long N, float* __restrict__ cb) {
    I3D_CHAIN_PRIO();
    __shared__ double sm[PC_COL_L][PC_COL_W];
    const int cx = threadIdx.x % PC_COL_W, ry = threadIdx.x / PC_COL_W;
    const long c = (long)blockIdx.x * PC_COL_W + cx;
    double acc = 0.;
    if (c < N) {
        const double b = (double)n2[c];
        for (long r = ry; r < B; r += PC_COL_L) {
            const double a = (double)n1[r];
            acc -= (double)dsim[r * N + c] * ((double)sim[r * N + c] / (a * b)) * a;
        }
    }
    sm[ry][cx] = acc;
    __syncthreads();
    if (ry == 0 && c < N) {
        const double b = (double)n2[c];
        double t = 0.;
        for (int k = 0; k < PC_COL_L; ++k) t += sm[k][cx];
        cb[c] = b > 0. ? (float)(t / b) : 0.f;
    }
}

}  // namespace i3d

using namespace i3d;

extern "C" int i3d_conf_match_max_conformers(void) { return CM_MAX_CONF; }
extern "C" int i3d_per_conf_max_conformers(void) { return PC_MAX_CONF; }

static int conf_match_check(int batch, int conf, int mode, float tau) {
    I3D_CHECK_ARG(batch >= 2, "fewer than two molecules");
    I3D_CHECK_ARG(conf >= 1 && conf <= CM_MAX_CONF, "conformers per molecule outside 1..8");
    I3D_CHECK_ARG((long)batch * conf <= 46340, "batch * conformers above 46340: the [BC, BC] matrix would pass 2^31 entries");
    I3D_CHECK_ARG(mode == CM_MIN || mode == CM_MAX, "mode is neither 0 (minimum matching) nor 1 (maximum similarity)");
    I3D_CHECK_ARG(tau > 0.f, "tau must be positive");
    return I3D_OK;
}

// floats of `work`: four [B, B] float tables, three [B] float vectors, one [B, B] byte table
extern "C" long i3d_conf_match_work_floats(int batch) {
    if (batch < 0) return 0;
    const long bb = (long)batch * batch;
    return 4 * bb + 3L * batch + (bb + 3) / 4;
}

extern "C" int i3d_conf_match_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, int mode, float tau,
                                  unsigned char* sel, unsigned char* dsel, double* row_den, double* row_pos, int* pos_j,
                                  int* pos_lu, float* loss, void* stream) {
    if (int rc = conf_match_check(batch, conf, mode, tau)) return rc;
    I3D_CHECK_ARG(sim && n1 && n2 && sel && row_den && row_pos && pos_j && pos_lu && loss, "null pointer");
    I3D_CHECK_ARG(mode != CM_MIN || dsel, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const double inv_tau = 1. / (double)tau;
    hipLaunchKernelGGL(cm_pair_kernel, dim3(cdiv((long)batch * batch, 4)), dim3(256), 0, s, sim, n1, n2, batch, conf, mode, sel, dsel);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cm_row_kernel, dim3(batch), dim3(256), 0, s, sim, n1, n2, batch, conf, mode, inv_tau, sel, dsel, row_den,
                       row_pos, pos_j, pos_lu);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cm_loss_kernel, dim3(1), dim3(256), 0, s, row_den, row_pos, batch, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_conf_match_bwd(const float* sim, const float* z1v, const float* z2, const float* n1, const float* n2,
                                  const unsigned char* sel, const double* row_den, const int* pos_j, const int* pos_lu, int batch,
                                  int conf, int dim, int mode, int norm, float tau, const float* grad_scale, float* work, float* dz1,
                                  float* dz2, void* stream) {
    if (int rc = conf_match_check(batch, conf, mode, tau)) return rc;
    I3D_CHECK_ARG(dim >= 1, "feature count below 1");
    I3D_CHECK_ARG(sim && z1v && z2 && n1 && n2 && sel && row_den && pos_j && pos_lu && work && dz1 && dz2, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long bb = (long)batch * batch;
    float* wz = work;
    float* wsa = wz + bb;
    float* wzT = wsa + bb;
    float* wsbT = wzT + bb;
    float* pwz = wsbT + bb;
    float* pwsa = pwz + batch;
    float* pwsb = pwsa + batch;
    unsigned char* selT = (unsigned char*)(pwsb + batch);
    hipLaunchKernelGGL(cm_weight_kernel, dim3(cdiv(bb, 256)), dim3(256), 0, s, sim, n1, n2, sel, row_den, pos_j, pos_lu, batch, conf,
                       norm, 1. / (double)tau, grad_scale, wz, wsa, wzT, wsbT, selT, pwz, pwsa, pwsb);
    I3D_CHECK_LAUNCH();
    const dim3 grid(batch, cdiv(dim, 256));
    hipLaunchKernelGGL(cm_gather_kernel<true>, grid, dim3(256), 0, s, z1v, z2, wz, wsa, sel, pos_j, pos_lu, pwz, pwsa, batch, conf, dim,
                       dz1);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cm_gather_kernel<false>, grid, dim3(256), 0, s, z2, z1v, wzT, wsbT, selT, pos_j, pos_lu, pwz, pwsb, batch, conf,
                       dim, dz2);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

static int per_conf_check(int batch, int conf, int mode, float tau) {
    I3D_CHECK_ARG(batch >= 2, "fewer than two molecules");
    I3D_CHECK_ARG(conf >= 1 && conf <= PC_MAX_CONF, "conformers per molecule outside 1..64");
    I3D_CHECK_ARG((long)batch * batch * conf < (1L << 31), "batch^2 * conformers at or above 2^31 entries");
    I3D_CHECK_ARG(mode == PC_V2 || mode == PC_V3, "mode is neither 0 (V2) nor 1 (V3)");
    I3D_CHECK_ARG(tau > 0.f, "tau must be positive");
    return I3D_OK;
}

extern "C" int i3d_per_conf_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, int mode, float tau,
                                double* den, double* pos, float* loss, void* stream) {
    if (int rc = per_conf_check(batch, conf, mode, tau)) return rc;
    I3D_CHECK_ARG(sim && n1 && n2 && den && pos && loss, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const double inv_tau = 1. / (double)tau;
    if (mode == PC_V3) hipLaunchKernelGGL(pc_fwd_kernel<true>, dim3(batch), dim3(256), 0, s, sim, n1, n2, batch, conf, inv_tau, den, pos);
    else hipLaunchKernelGGL(pc_fwd_kernel<false>, dim3(batch), dim3(256), 0, s, sim, n1, n2, batch, conf, inv_tau, den, pos);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cm_loss_kernel, dim3(1), dim3(256), 0, s, den, pos, mode == PC_V3 ? batch * conf : batch, loss);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}

extern "C" int i3d_per_conf_bwd(const float* sim, const float* n1, const float* n2, const double* den, const double* pos, int batch,
                                int conf, int mode, float tau, const float* grad_scale, float* dsim, float* ca, float* cb,
                                void* stream) {
    if (int rc = per_conf_check(batch, conf, mode, tau)) return rc;
    I3D_CHECK_ARG(sim && n1 && n2 && den && pos && dsim && ca && cb, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    const double inv_tau = 1. / (double)tau;
    const long N = (long)batch * conf;
    if (mode == PC_V3)
        hipLaunchKernelGGL(pc_bwd_row_kernel<true>, dim3(batch), dim3(256), 0, s, sim, n1, n2, den, pos, batch, conf, inv_tau,
                           grad_scale, dsim, ca);
    else
        hipLaunchKernelGGL(pc_bwd_row_kernel<false>, dim3(batch), dim3(256), 0, s, sim, n1, n2, den, pos, batch, conf, inv_tau,
                           grad_scale, dsim, ca);
    I3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pc_bwd_col_kernel, dim3(cdiv(N, PC_COL_W)), dim3(256), 0, s, sim, dsim, n1, n2, batch, N, cb);
    I3D_CHECK_LAUNCH();
    return I3D_OK;
}
