/* lib3dinfomax_hip.so - C ABI of the MI355X (gfx950) kernels behind the 3DInfomax pre-training hot path.
 *
 * The reference (HannesStark/3DInfomax) is pure Python: its "FFI" for this path is the set of ATen/DGL
 * calls its nn.Modules make.  Every entry point below replaces one such call site (cited as
 * reference file:line) and is what a maintainer binds with ctypes (the in-tree
 * binding is 3dinfomax_amd/_lib.py + ops.py).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless the parameter comment says
 *    "host"; tensors are dense row-major fp32 unless stated; index arrays are int32.
 *  - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all work is enqueued
 *    asynchronously on it, nothing synchronises the device, no hidden allocations except where a
 *    `workspace` pointer is taken explicitly.
 *  - return value: I3D_OK (0) or a negative I3D_ERR_*; i3d_last_error() returns a thread-local message.  The entry points that
 *    say so return I3D_NOT_TAKEN (1) for a valid call outside what their kernels cover: nothing was launched, nothing written.
 *  - edge-sized tensors are in DESTINATION-SORTED ("epos") order: the in-edges of node v are the
 *    contiguous rows [in_ptr[v], in_ptr[v+1]) (stable w.r.t. edge id = DGL's mailbox order).
 *  - thread safety: the error string is thread-local.  PROCESS-WIDE state exists and is set through explicit setters only:
 *    the fp32 product form (i3d_set_fp32_products), the one-launch BatchNorm backward (i3d_set_bn_bwd_one_launch), the
 *    collective table of synchronised BatchNorm (i3d_set_collectives / the peer exchange) and the per-stream side-stream
 *    table; call the setters before the first compute call of the other threads.
 */
#ifndef INFOMAX3D_HIP_H
#define INFOMAX3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I3D_OK 0
#define I3D_ERR_INVALID (-1)
#define I3D_ERR_LAUNCH (-2)
#define I3D_NOT_TAKEN 1

/* activations: reference models/base_layers.py:9-20 (get_activation) */
#define I3D_ACT_NONE 0
#define I3D_ACT_RELU 1
#define I3D_ACT_SILU 2
#define I3D_ACT_SIGMOID 3
#define I3D_ACT_LEAKY_RELU 4 /* negative slope 0.01 = nn.LeakyReLU() default, reference models/pna_original.py:291 */
/* the rest of the reference's SUPPORTED_ACTIVATION_MAP (models/base_layers.py:5) with torch's default parameters; GLU (halves the
 * feature dimension) is not an elementwise activation and is not offered */
#define I3D_ACT_TANH 5
#define I3D_ACT_ELU 6      /* alpha 1 */
#define I3D_ACT_SELU 7
#define I3D_ACT_SOFTPLUS 8 /* beta 1, threshold 20 */

/* aggregators: reference models/pna.py:71-81 (PNA_AGGREGATORS); readout ops: dgl.readout_nodes */
#define I3D_AGG_MEAN 0
#define I3D_AGG_SUM 1
#define I3D_AGG_MAX 2
#define I3D_AGG_MIN 3
#define I3D_AGG_STD 4
#define I3D_AGG_VAR 5

/* scalers: reference models/pna.py:83-87 (PNA_SCALERS) */
#define I3D_SCALE_IDENTITY 0
#define I3D_SCALE_AMPLIFICATION 1
#define I3D_SCALE_ATTENUATION 2

int i3d_abi_version(void); /* 2 (1 -> 2: I3dBnTail lost its last member, the deferred-bias entry points are gone) */
const char* i3d_last_error(void);

/* ---- K1: fused multi-table embedding sum -----------------------------------------------------------
 * replaces AtomEncoder.forward / BondEncoder.forward, reference commons/mol_encoder.py:34-42, 65-73
 * (n_cols nn.Embedding lookups + adds).  out[r,:] = sum_k tables[k][idx[r,k], :].
 *   idx     int64 [rows, n_cols]          tables  host array of n_cols device pointers, table k is [dim_k, feat]
 *   row_perm int32 [rows] or NULL: output row r uses index row row_perm[r] (bond features are stored in edge-id
 *            order, the kernels want destination-sorted edges: the permutation is folded into the lookup)
 * bwd: grad_tables[k][idx[r,k], :] += grad_out[r,:]  (caller zero-fills; dims = host array of table sizes,
 * sum(dims)*feat*4 bytes must fit the 160 KiB LDS of a CU for the LDS-privatised path, else global atomics). */
int i3d_embedding_sum_fwd(const int64_t* idx, const int* row_perm, int rows, int n_cols, const float* const* tables,
                          int feat, float* out, void* stream);
int i3d_embedding_sum_bwd(const int64_t* idx, const int* row_perm, int rows, int n_cols, const float* grad_out,
                          int feat, float* const* grad_tables, const int* dims, void* stream);

/* ---- K4: PNA aggregation (the HBM-roofline kernel) -------------------------------------------------
 * replaces DGL update_all(message_func, reduce_func) + aggregators + scalers,
 * reference models/pna.py:206, 215-235, 17-37, 57-68.
 *   e [E, feat] messages in epos order;  in_ptr [N+1];  aggregators/scalers: host int arrays (I3D_AGG_*, I3D_SCALE_*)
 *   out [N, n_scalers_eff * n_aggregators * feat], scaler-major, zero rows for in-degree 0;
 *   n_scalers_eff = n_scalers if n_scalers > 1 else 1 with NO scaling (reference quirk, models/pna.py:232).
 *   force_scalers != 0: apply the scalers also when only one is configured (reference models/pna_original.py:235,
 *   422 - the original PNA layers have no such quirk).
 *   avg_d_log: the reference hard-codes 1.0 (models/pna.py:153); pna_original.py passes the real value.
 * bwd: grad_e [E, feat] (fully overwritten).  max/min ties route to the first (lowest edge id) slot. */
int i3d_pna_aggregate_fwd(const float* e, const int* in_ptr, int num_nodes, int feat, const int* aggregators,
                          int n_aggregators, const int* scalers, int n_scalers, int force_scalers, float avg_d_log,
                          float* out, void* stream);
int i3d_pna_aggregate_bwd(const float* grad_out, const float* e, const int* in_ptr, int num_nodes, int feat,
                          const int* aggregators, int n_aggregators, const int* scalers, int n_scalers,
                          int force_scalers, float avg_d_log, float* grad_e, void* stream);

/* ---- K6: per-graph readout -------------------------------------------------------------------------
 * replaces dgl.readout_nodes(graph,'feat',op) for op in readout_aggregators + torch.cat,
 * reference models/pna.py:133-134, models/net3d.py:73-74.
 *   x [N, feat]; graph_ptr [B+1] node offsets; ops host array of I3D_AGG_{MEAN,SUM,MAX,MIN}
 *   out [B, n_ops*feat].  bwd: grad_x [N, feat] (fully overwritten), ties -> first node. */
int i3d_segment_readout_fwd(const float* x, const int* graph_ptr, int num_graphs, int feat, const int* ops,
                            int n_ops, float* out, void* stream);
int i3d_segment_readout_bwd(const float* grad_out, const float* x, const int* graph_ptr, int num_graphs, int feat,
                            const int* ops, int n_ops, float* grad_x, void* stream);

/* ---- dense towers: fp32 MFMA GEMM ------------------------------------------------------------------
 * replaces nn.Linear forward/backward inside FCLayer, reference models/base_layers.py:101 (aten::addmm/mm).
 *   C[M,N] (ldc) = (accumulate ? C : 0) + opA(A)[M,K] * opB(B)[K,N] + (bias ? bias[N] : 0)
 *   trans_a = 0: A stored [M,K] (lda >= K);  1: A stored [K,M] (lda >= M)
 *   trans_b = 0: B stored [K,N] (ldb >= N);  1: B stored [N,K] (ldb >= K)
 * exact fp32 (v_mfma_f32_16x16x4_f32), fp32 accumulate.
 *   Linear fwd  Y = X W^T + b : trans_a=0, trans_b=1, B=W[N,K]
 *   dX = dY W               : trans_a=0, trans_b=0, B=W
 *   dW = dY^T X             : trans_a=1, trans_b=0, A=dY[M',N'] (K := rows) */
int i3d_gemm_f32(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                 float* C, int ldc, const float* bias, int accumulate, void* stream);
/* tuning entry: same, with the tile configuration BMxBNxBK forced (0: 128x128x16, 1: 256x32x16, 2: 64x64x16, 3: 32x64x32 on
 * v_mfma_f32_16x16x4_f32; 4: 64x64x16, 5: 128x128x16 on v_mfma_f32_32x32x2_f32; -1 = auto) and the split-K factor
 * (0 = auto) - used by tools/gemm_bench.py to pick the dispatch heuristics */
int i3d_gemm_f32_ex(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, const float* bias, int accumulate, int tile_cfg, int splits, void* workspace,
                    long workspace_bytes, void* stream);
/* Precision of every GEMM of the library (process-level; the reference's switch is the trainer's `dtype`, configs[3] of
 * BASELINE.json): 0 (default) = exact fp32 products on the fp32 matrix pipe; 1 = the operands are rounded to bf16
 * (round-to-nearest-even) as a lane reads its fragments and multiplied with v_mfma_f32_*_bf16, accumulation / bias /
 * epilogue / BatchNorm statistics / tensors in memory stay fp32 (the master weights are the fp32 parameters). */
int i3d_set_matmul_precision(int bf16);
int i3d_get_matmul_precision(void);
/* fp32 mode only - how the tiled forward / data-gradient GEMMs (32x32 MFMA tiles, 16-byte aligned operands) form the product of
 * two fp32 operands: 0 = v_mfma_f32_32x32x2_f32; 1 = both operands split exactly into three bf16 parts (x = hi + mid + lo) and
 * the six part products of order <= 2 taken on the bf16 matrix pipe with fp32 accumulation (each part product is exact; what is
 * dropped is <= 3 x 2^-24 |a b|, the size of one fp32 rounding) - the same nn.Linear arithmetic class as
 * /root/reference/models/base_layers.py:101, 2.7x fewer matrix-pipe cycles.  Process-level; I3D_FP32_PRODUCTS=native|split
 * sets it at load.  THE LIBRARY DEFAULT IS 1 (split) - every "fp32" result of this library (tests, bench.py's headline) is formed
 * this way unless 0 is set; the weight-gradient panels (wgrad.hip) and the small-tile / unaligned kernels always use the fp32
 * pipe.  Non-finite and huge operands: the split is exact for |x| <= 3.39e38 (above it the bf16 rounding of `hi` overflows); an
 * operand that is +-Inf or beyond that bound gives hi = +-Inf and a NaN remainder, so the outputs that depend on it are NaN where
 * the fp32 pipe gives +-Inf (or NaN): they are non-finite in exactly the positions where the native product is non-finite, but
 * isinf() does not tell overflow from invalid any more (tests/test_gpu_ops.py: test_split_products_with_non_finite_operands). */
int i3d_set_fp32_products(int split);
int i3d_get_fp32_products(void);

/* Row-panel form of the chain's Linear products (csrc/panel.hip; reference models/base_layers.py:101 and its data gradient): the
 * weight is split ONCE per optimisation step into the three bf16 images of the split form (i3d_set_fp32_products) and laid out as the
 * LDS image of the product kernel - i3d_panel_pack: trans 1 = B[n][k] = W[n * ldw + k] (forward, W stored [out, in]), 0 = B[n][k] =
 * W[k * ldw + n] (data gradient); `packed`: i3d_panel_packed_bytes(N, K) bytes, 16-byte aligned - and i3d_panel_gemm forms
 * C[M, N] (+)= A[M, K] B^T (+ bias) with every 64-row slab of A read and split once per 208-column block.  K % 8 == 0, N % 4 == 0,
 * 16-byte aligned rows.  Same arithmetic as the split form of i3d_gemm_f32 (six bf16 part products, fp32 accumulation). */
long i3d_panel_packed_bytes(int N, int K);
int i3d_panel_pack(const float* W, int ldw, int N, int K, int trans, void* packed, void* stream);
typedef struct {
    const float* W;
    int ldw, N, K, trans;
    void* packed;
} I3dPanelPack;
int i3d_panel_pack_multi(const I3dPanelPack* weights, int n, void* stream); /* up to 8 weights (a layer's) in ONE launch */
int i3d_panel_gemm(int M, int N, int K, const float* A, int lda, const void* packed, float* C, int ldc, const float* bias,
                   int accumulate, void* stream);
/* the fused forward of a block behind a never-materialised BatchNorm (i3d_gemm_f32_fused in row-panel form): A read as
 * (A - mean) * scale + shift (a_aff [3 K], may be NULL), the stored value = act(product + bias), and - stats != NULL - per 32-row
 * tile and column {sum, M2 about the tile mean, row count} of the stored values: stats [i3d_panel_stats_tiles(M)][3][N] */
int i3d_panel_stats_tiles(int M);
int i3d_panel_gemm_fused(int M, int N, int K, const float* A, int lda, const void* packed, float* C, int ldc, const float* bias,
                         const float* a_aff, int epi_act, float* stats, void* stream);

/* i3d_gemm_f32 with scratch: when the reduction dimension is split over workgroups (weight gradients), the slices are
 * written to workspace[slices][M][N] and summed in a fixed order by a second kernel (deterministic, no zero-fill, no
 * atomics).  workspace NULL or too small: fp32 atomics as i3d_gemm_f32. */
int i3d_gemm_f32_ws(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, const float* bias, int accumulate, void* workspace, long workspace_bytes,
                    void* stream);

/* i3d_gemm_f32_ws where B and/or C consist of two blocks of one parent matrix (the [W_s | W_d] column blocks of an
 * edge-MLP weight, P trick of i3d_edge_combine_fwd: P = h [W_s | W_d]^T, dh = dP [W_s; W_d], d[W_s | W_d] = dP^T h as ONE
 * GEMM each instead of two):  B index (n if trans_b, k otherwise) >= b_split adds b_delta floats to the address and
 * b_view_floats is the number of floats addressable behind B; C rows >= c_split add c_delta floats.  b_split / c_split
 * <= 0: plain operand. */
int i3d_gemm_f32_blocks(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        int b_split, long b_delta, long b_view_floats, float* C, int ldc, int c_split, long c_delta,
                        int accumulate, void* workspace, long workspace_bytes, void* stream);

/* K4 with a tower-major row layout (the tower variant's stacked layers, csrc/tower.hip): the feat message columns are feat /
 * tower_feat towers; a node's output row is [tower][block (scaler, aggregator)][feature of the tower] instead of
 * [block][feature] - the B blocks of one tower are one contiguous column range.  feat % 4 == tower_feat % 4 == 0; otherwise as
 * i3d_pna_aggregate_fwd / _bwd (grad_out in the same layout). */
int i3d_pna_aggregate_fwd_towers(const float* e, const int* in_ptr, int num_nodes, int feat, int tower_feat,
                                 const int* aggregators, int n_aggregators, const int* scalers, int n_scalers,
                                 int force_scalers, float avg_d_log, float* out, void* stream);
int i3d_pna_aggregate_bwd_towers(const float* grad_out, const float* e, const int* in_ptr, int num_nodes, int feat,
                                 int tower_feat, const int* aggregators, int n_aggregators, const int* scalers,
                                 int n_scalers, int force_scalers, float avg_d_log, float* grad_e, void* stream);
/* n_batch products of ONE shape in one launch: batch b multiplies A + b a_batch by B + b b_batch into C + b c_batch (strides in
 * floats; layouts and `accumulate` as i3d_gemm_f32, no bias; K-slices of weight-gradient layouts go through `workspace` as in
 * i3d_gemm_f32_ws and are required to: n_batch <= 32).  The diagonal blocks of a block-diagonal product: the posttrans Linear of
 * the `towers` PNATowers of a layer (reference models/pna_original.py:209-211, 250: tower t reads only ITS aggregated columns),
 * forward, data gradient and weight gradient, without the zero blocks of the stacked weight (csrc/tower.hip). */
int i3d_gemm_f32_batched(int trans_a, int trans_b, int M, int N, int K, const float* A, int lda, long a_batch, const float* B,
                         int ldb, long b_batch, float* C, int ldc, long c_batch, int n_batch, int accumulate, void* workspace,
                         long workspace_bytes, void* stream);

/* i3d_gemm_f32_grouped (below) whose per-group weight is block-diagonal: batch b multiplies the columns A + b a_batch of the
 * group's rows by B_g + b b_batch into the columns C + b c_batch - the towers' blocks of the per-degree posttrans weights of the
 * tower variant (csrc/tower.hip with I3dTowerLayerArgs.n_towers > 1 and n_deg_groups > 0) */
int i3d_gemm_f32_grouped_batched(int trans_b, int m_padded, int N, int K, const float* A, int lda, long a_batch, long a_rows_total,
                                 const int* m_rows, const int* tile_group, const float* B, int ldb, long b_group_stride, long b_batch,
                                 float* C, int ldc, long c_batch, int n_batch, int accumulate, void* stream);

/* ---- degree-grouped posttrans of the PNA layer ------------------------------------------------------
 * replaces cat([h, agg]) -> posttrans Linear of reference models/pna.py:207-209 for the aggregated part:  the three
 * scaler blocks of agg are per-node multiples (functions of the in-degree D only) of the same aggregator block a,
 * so  [a | amp(D) a | att(D) a] W_agg^T = a W_D^T  with  W_D = sum_s c_s(D) W_s  (re-association only): K drops
 * from n_scalers*A to A, and the aggregation kernel only has to write the identity block.
 *  combine_weights_fwd: WD[g, n, k] = sum_s coef[g*n_scalers+s] * W[n, f_in + s*agg_width + k]   (coef: host array)
 *  combine_weights_bwd: dW[n, f_in + s*agg_width + k] = sum_g coef[g*n_scalers+s] * dWD[g, n, k]
 *  gemm_f32_grouped:    C[r, :] (+)= A[r, :] * op(B_g) for r = m_rows[m] >= 0, g = tile_group[m / 64]; m_rows lists
 *                       the nodes grouped by in-degree, every group padded with -1 to a multiple of 64 rows;
 *                       trans_b = 1: B_g stored [N, K] (forward, B_g = WD[g]);  0: B_g stored [K, N] (data gradient)
 *  gemm_f32_rowsubset:  C[M, N] = sum_j A[k_rows[j], 0:M]^T B[k_rows[j], 0:N]   (weight gradient of one group)
 *  gemm_f32_rowsubset_multi: the same for n_groups disjoint ranges [group_start[g], +group_count[g]) of k_rows in ONE
 *                       launch, C_g = C + g * c_group_stride (host arrays for the ranges; tile_cfg -1 / seg_rows 0 =
 *                       automatic; the row segments are combined through `workspace` like i3d_gemm_f32_ws, or with
 *                       fp32 atomics when it is NULL / too small) */
int i3d_pna_combine_weights_fwd(const float* W, int ldw, int f_in, int f_out, int agg_width, int n_groups,
                                int n_scalers, const float* coef, float* WD, void* stream);
int i3d_pna_combine_weights_bwd(const float* dWD, int ldw, int f_in, int f_out, int agg_width, int n_groups,
                                int n_scalers, const float* coef, float* dW, void* stream);
int i3d_gemm_f32_grouped(int trans_b, int m_padded, int N, int K, const float* A, int lda, long a_rows_total,
                         const int* m_rows, const int* tile_group, const float* B, int ldb, long b_group_stride,
                         float* C, int ldc, int accumulate, void* stream);
int i3d_gemm_f32_rowsubset(int M, int N, int n_rows, const float* A, int lda, const float* B, int ldb,
                           const int* k_rows, long rows_total, float* C, int ldc, int accumulate, void* stream);
int i3d_gemm_f32_rowsubset_multi(int M, int N, int n_groups, const int* group_start, const int* group_count,
                                 const float* A, int lda, const float* B, int ldb, const int* k_rows, long rows_total,
                                 float* C, long c_group_stride, int ldc, int accumulate, int tile_cfg, int seg_rows,
                                 void* workspace, long workspace_bytes, void* stream);

/* ---- column statistics / BatchNorm1d ---------------------------------------------------------------
 * replaces nn.BatchNorm1d in FCLayer (train: batch statistics, momentum m, unbiased running_var; eval: running
 * statistics), reference models/base_layers.py:87, 106-110, plus the activation in front of it (:102-103).
 *
 * i3d_act_stats_fwd: x = act(pre) written to `x` (may alias pre; pass act NONE and x == pre for stats only),
 *   then mean[feat], invstd[feat] = 1/sqrt(biased var + eps); if running_mean != NULL the running statistics are
 *   updated in place (running = (1-m)*running + m*batch, var unbiased).  `count_extra`/`stats_extra` support
 *   synchronised BN: when sums_out != NULL the kernel only writes the fp64 sums_out[2*feat+1] = {sum x,
 *   sum x^2, rows} and does NOT finalise (the caller all-reduces them and calls i3d_bn_finalize_stats).
 *   workspace: device scratch of i3d_colreduce_workspace_bytes(rows, feat) bytes, ZERO-INITIALISED once by the caller
 *   and used by one stream at a time: the column reductions (this function, i3d_bn_bwd, i3d_bn_eval_bwd, i3d_colsum)
 *   are two-stage and deterministic.  With I3D_FUSED_FINAL=1 in the environment the second stage runs inside the first
 *   stage's launch (the last workgroups to arrive reduce the partial rows), synchronised through two counters at the
 *   head of the workspace that every launch leaves at zero; by default it is a separate small launch. */
long i3d_colreduce_workspace_bytes(int rows, int feat);
int i3d_act_stats_fwd(const float* pre, int rows, int feat, int act, float* x, float eps, float momentum,
                      float* mean, float* invstd, float* running_mean, float* running_var, double* sums_out,
                      void* workspace, void* stream);
/* as i3d_act_stats_fwd; additionally increments *num_batches_tracked (BatchNorm1d's int64 counter, may be NULL) in the
 * kernel that updates the running statistics - reference models/base_layers.py:107-108 runs nn.BatchNorm1d in training
 * mode, which bumps it once per forward */
int i3d_act_stats_fwd_counted(const float* pre, int rows, int feat, int act, float* x, float eps, float momentum,
                      float* mean, float* invstd, float* running_mean, float* running_var, double* sums_out, long long* num_batches_tracked,
                      void* workspace, void* stream);
/* fp64 sums [2*feat+1] = {sum x, sum x^2, count} (already all-reduced) -> mean, invstd, running stats update */
int i3d_bn_finalize_stats(const double* sums, int feat, float eps, float momentum, float* mean, float* invstd,
                          float* running_mean, float* running_var, void* stream);
/* y = post_act( (x-mean)*invstd*gamma + beta ) + (residual ? residual : 0).   y may alias x. */
int i3d_bn_apply_fwd(const float* x, int rows, int feat, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, int post_act, const float* residual, float* y,
                     void* stream);
/* eval mode: invstd computed from running_var on the fly */
int i3d_bn_eval_fwd(const float* x, int rows, int feat, const float* running_mean, const float* running_var,
                    float eps, const float* gamma, const float* beta, int post_act, const float* residual, float* y,
                    void* stream);
/* backward of  y = post_act(BN(x)), x = act(pre)   (train mode):
 *   grad_y, x [rows,feat]; pre may be NULL when act is NONE or RELU (x itself decides relu');
 *   outputs: grad_gamma[feat], grad_beta[feat], grad_pre [rows,feat] (may alias grad_y).
 *   If sums_out != NULL: phase 1 only - writes the LOCAL grad_gamma/grad_beta and the fp64 sums_out[2*feat] =
 *   {sum dy, sum dy*xhat} for the sync-BN all-reduce (the caller stores its row count in sums[2*feat] before
 *   reducing); then call again with sums_in != NULL (phase 2: the reduced sums and the count sums_in[2*feat]
 *   drive grad_pre - total_rows is ignored, nothing is read back to the host; grad_gamma/grad_beta untouched).   grad_bias (may be NULL): column sums of grad_pre - the bias gradient of the Linear in
 * front of the block - from the same pass that writes grad_pre. */
int i3d_bn_bwd(const float* grad_y, const float* x, const float* pre, int rows, int feat, int act, int post_act,
               const float* mean, const float* invstd, const float* gamma, const float* beta, float* grad_gamma,
               float* grad_beta, float* grad_pre, float* grad_bias, double* sums_out, const double* sums_in,
               long total_rows, void* workspace, void* stream);
/* eval-mode backward (statistics are constants): grad_pre = grad_y * post_act' * gamma*invstd * act' */
int i3d_bn_eval_bwd(const float* grad_y, const float* x, const float* pre, int rows, int feat, int act,
                    int post_act, const float* running_mean, const float* running_var, float eps,
                    const float* gamma, const float* beta, float* grad_gamma, float* grad_beta, float* grad_pre,
                    void* workspace, void* stream);
/* out[feat] = sum over rows of x[r,:] * (w ? w[r] : 1)   (bias gradients, weighted column sums) */
int i3d_colsum(const float* x, const float* w, int rows, int feat, float* out, void* workspace, void* stream);
/* y = act(x) elementwise (n elements); bwd: grad_x = grad_y * act'(x) */
int i3d_act_fwd(const float* x, long n, int act, float* y, void* stream);
int i3d_act_bwd(const float* grad_y, const float* x, long n, int act, float* grad_x, void* stream);
/* The gates of ONE GRU step (csrc/gru.hip) - reference models/pna_original.py:64-84 (`GRU`: nn.GRU run for one step between the layers
 * of PNAGNNOriginal with gru_enable=True, :190-193).  GI = x W_ih^T + b_ih, GH = h0 W_hh^T + b_hh [rows, 3 hidden] (gate order r | z | n,
 * torch's); forward: out = (1 - z) n + z h0, saved [rows, 3 hidden] = r | z | n; backward: gradients w.r.t. GI, GH and the direct
 * share of h0 (the caller adds grad_GH W_hh). */
int i3d_gru_gates_fwd(const float* GI, const float* GH, const float* h0, int rows, int hidden, float* out, float* saved, void* stream);
int i3d_gru_gates_bwd(const float* grad_out, const float* saved, const float* GH, const float* h0, int rows, int hidden, float* grad_GI,
                      float* grad_GH, float* grad_h0, void* stream);
/* dst += src;  out = a + b;  out[r, :] = row for r < rows (Net3D's broadcast node embedding, models/net3d.py:61) */
int i3d_add_inplace(float* dst, const float* src, long n, void* stream);
int i3d_add(const float* a, const float* b, long n, float* out, void* stream);
/* out = a * b elementwise (out may alias a): nn.Dropout of FCLayer / the tower variants with the scaled mask as b (reference
 * models/base_layers.py:84-85, 104-105; models/pna_original.py:260, 428) */
int i3d_mul(const float* a, const float* b, long n, float* out, void* stream);
int i3d_broadcast_row(const float* row, long rows, int feat, float* out, void* stream);

/* ---- edge kernels ----------------------------------------------------------------------------------
 * i3d_edge_combine_fwd replaces the gather + concat + first Linear of the edge MLPs,
 *   reference models/pna.py:237-252 (pretrans_edges: cat[h_src, h_dst, e_feat] -> Linear) and
 *   models/net3d.py:113-115, using  [h_s|h_d|q] W^T = h_s W_s^T + h_d W_d^T + q W_q^T :
 *   pre[j,:] = P[src_s[j], 0:feat] + P[dst_s[j], feat:2feat] + Q[q_code ? q_code[j] : j,:] + bias
 *   (P is [N, ldp >= 2*feat]; Q, q_code, bias may be NULL)
 * i3d_edge_codes: categorical edge features with a small joint vocabulary V (bonds, commons/mol_encoder.py:45-73:
 *   5 x 6 x 2 = 60): codes[j] = sum_c idx[row_perm ? row_perm[j] : j, c] * strides[c] (host array), and the one-hot
 *   matrix onehot[rows, v_pad] (v_pad >= V, multiple of 4).  The bond embedding of an edge is then row codes[j] of the
 *   [V, F] table of all combinations, so the per-layer  e_feat W_q^T  is a gather from (table W_q^T) (q_code above)
 *   and its gradients are  onehot^T dpre  ([V, F] instead of two [E, F] x [F, F] products).
 * i3d_segment_sum: out[v,:] = scale(v) * sum_{j in [ptr[v],ptr[v+1])} x[idx ? idx[j] : j, :]
 *   scale_mode 0: 1;  1: 1/max(count,1)  (DGL fn.mean, reference models/net3d.py:95-96)
 *   used for the backward of the gathers (by in_ptr, and by out_ptr/out_epos) and for Net3D's mean reduce.
 * i3d_segment_bcast: grad of segment mean/sum: out[j,:] = scale(seg(j)) * g[seg(j),:], seg given by dst_s. */
int i3d_edge_combine_fwd(const float* P, int ldp, const float* Q, const int* q_code, const float* bias,
                         const int* src_s, const int* dst_s, int num_edges, int feat, float* pre, void* stream);
/* multi-hot encoding of categorical columns: out[j, offsets[c] + idx[row_perm ? row_perm[j] : j, c]] = 1, else 0
 * (out [rows, v_pad], offsets: host prefix sums of the table sizes).  out^T dY is the gradient of all embedding tables of
 * an encoder (commons/mol_encoder.py:34-42) as one weight-gradient GEMM - deterministic, unlike the atomics of
 * i3d_embedding_sum_bwd. */
int i3d_multihot(const int64_t* idx, const int* row_perm, int rows, int n_cols, const int* offsets, int v_pad, float* out,
                 void* stream);
int i3d_edge_codes(const int64_t* idx, const int* row_perm, int rows, int n_cols, const int* strides, int v_pad,
                   int* codes, float* onehot, void* stream);
int i3d_segment_sum(const float* x, int ldx, const int* ptr, const int* idx, int num_segments, int feat,
                    int scale_mode, float* out, int ldo, void* stream);
/* two segmentations of the same rows in one launch (sums, no scaling): out0 over (ptr0, idx0), out1 over (ptr1, idx1) */
/* i3d_segment_sum over rows of bf16 values (x: row r at (bf16*)x + r * ldx; feat, ldx multiples of 4, 8-byte aligned), fp32 sums */
int i3d_segment_sum_bf16(const void* x, int ldx, const int* ptr, const int* idx, int num_segments, int feat, int scale_mode,
                         float* out, int ldo, void* stream);
int i3d_segment_sum_pair(const float* x, int ldx, const int* ptr0, const int* idx0, float* out0, const int* ptr1,
                         const int* idx1, float* out1, int num_segments, int feat, int ldo, void* stream);
int i3d_segment_bcast(const float* g, const int* ptr, const int* seg_of_row, int rows, int feat, int scale_mode,
                      float* out, void* stream);
/* rows gather: out[j,:] = x[idx[j],:]  (edge permutation edge-id -> epos order) */
int i3d_gather_rows(const float* x, const int* idx, int rows, int feat, float* out, void* stream);

/* ---- Net3D specifics -------------------------------------------------------------------------------
 * fourier: replaces fourier_encode_dist, reference commons/utils.py:103-110, models/net3d.py:63-64:
 *   out[j,:] = [sin(d/2^k)]_{k<n} | [cos(d/2^k)]_{k<n} | d        out [E, 2n+1]
 * soft edge gate: reference models/net3d.py:106, 117-118:  w = sigmoid(m . ws + bs);  msg = m * w
 *   bwd: grad_m [E,feat], g_gate[E] = (sum_f grad_msg*m) * w(1-w)  (so that grad_ws = sum_e g_gate*m, grad_bs = sum g_gate) */
int i3d_fourier_encode(const float* d, int num_edges, int n_enc, float* out, void* stream);
int i3d_soft_edge_fwd(const float* m, const float* ws, const float* bs, int num_edges, int feat, float* msg,
                      float* w, void* stream);
int i3d_soft_edge_bwd(const float* grad_msg, const float* m, const float* w, const float* ws, int num_edges,
                      int feat, float* grad_m, float* g_gate, void* stream);

/* ---- NT-Xent ---------------------------------------------------------------------------------------
 * replaces NTXent.forward / NTXentMultiplePositives.forward, reference commons/losses.py:143-155, 225-247.
 *   z1 [b1, dim] (local 2D-view rows), z2 [b2*conf, dim] (all 3D-view rows, conformer-minor); the positive columns
 *   of row i are (pos_offset+i)*conf .. +conf-1 (pos_offset = rank*b1 when z2 is the all-gathered batch).
 *   eps: 1e-8 for NTXent, 0 for the multiple-positives variant (reference :150 vs :239).
 *   sim  [b1, b2*conf] = z1 z2^T from i3d_gemm_f32;  dsim [b1, b2*conf] receives dL/dS
 *   fwd: loss_sum[0] = sum_i -log(pos_i / (rowsum_i - pos_i))   (caller divides by the GLOBAL batch size)
 *   bwd: writes dsim = dL/dS (scaled by grad_scale = upstream/global_batch) and the norm-path
 *        coefficients ca[b1], cb[b2*conf] such that dz1 = dS z2 + ca*z1, dz2 = dS^T z1 + cb*z2. */
int i3d_row_norms(const float* z, int rows, int dim, float* norms, void* stream);
/* loss_sum[0] = loss_scale * sum_i l_i (loss_scale = 1/global batch);  the backward multiplies by grad_scale and, when
 * grad_scale_dev != NULL, by the device scalar grad_scale_dev[0] (the upstream gradient of the loss: no host read-back) */
int i3d_ntxent_fwd(const float* sim, const float* n1, const float* n2, int b1, int b2, int conf, int pos_offset,
                   float tau, float eps, float loss_scale, float* row_sum, float* row_pos, float* loss_sum, void* stream);
int i3d_ntxent_bwd(const float* sim, const float* n1, const float* n2, const float* row_sum, const float* row_pos,
                   int b1, int b2, int conf, int pos_offset, float tau, float eps, float grad_scale,
                   const float* grad_scale_dev, float* dsim, float* ca, float* cb, void* stream);
/* the whole loss from one call per direction (row norms, similarity GEMM, i3d_ntxent_fwd / i3d_ntxent_bwd, the two
 * gradient GEMMs and their normalisation terms; reference commons/losses.py:143-155, 225-247).  scratch
 * (i3d_ntxent_loss_scratch_floats(b1, b2 * conf) floats) is written by the forward and read by the backward; work:
 * b1 * b2c + b1 + b2c (+ alignment) floats.  z1 [b1, dim] local rows, z2 [b2 * conf, dim] the (gathered) other view. */
long i3d_ntxent_loss_scratch_floats(int b1, int b2c);
int i3d_ntxent_loss_fwd(const float* z1, const float* z2, int b1, int b2, int conf, int dim, int pos_offset, float tau,
                        float eps, float loss_scale, float* scratch, float* loss, void* stream);
int i3d_ntxent_loss_bwd(const float* z1, const float* z2, int b1, int b2, int conf, int dim, int pos_offset, float tau,
                        float eps, float loss_scale, const float* scratch, const float* grad_scale_dev, float* work, float* dz1,
                        float* dz2, void* stream);
/* out[r,:] += coef[r] * z[r,:] */
int i3d_row_axpy(const float* z, const float* coef, int rows, int dim, float* out, void* stream);
/* out[r,:] = coef[r] * z[r,:]   (graph-size normalisation h * snorm_n, reference models/pna_original.py:258-259) */
int i3d_row_scale(const float* z, const float* coef, int rows, int dim, float* out, void* stream);
/* ---- the tower variant's stacked parameters (csrc/pack.hip; reference models/pna_original.py:264-319: `towers` PNATowers per
 * layer, outputs concatenated) - n_blocks 2-D copies src[rows, cols] (pitch ld_src) -> dst (pitch ld_dst) in ONE launch, the
 * table in device memory; reverse != 0: dst -> src (stacked gradients / running statistics back to the towers' tensors) */
typedef struct {
    const float* src;
    float* dst;
    int rows, cols;
    long ld_src, ld_dst;
} I3dCopyBlock;
int i3d_block_copy(const I3dCopyBlock* table /* device */, int n_blocks, int reverse, void* stream);
/* dst[rows, cols_dst] (contiguous) = the first cols_dst columns of src[rows, cols_src] (contiguous), zeros where cols_dst >
 * cols_src: the stacked towers run on activations whose width is rounded up to 4 floats (hidden_dim 90 of the reference's
 * configs/pna_original.yml -> 92: every kernel then takes its 16-byte form); the embedding's output is widened once, the
 * last layer's output cropped once, their gradients the other way round */
int i3d_copy_cols(const float* src, int rows, int cols_src, float* dst, int cols_dst, void* stream);
/* out[j * ld + col] = sum_k (x[src[j], k] - x[dst[j], k])^2 over the three coordinates of x [N, 3] - the squared distance that
 * PNALayer.pretrans_edges appends to an edge's features with pairwise_distances=True (reference models/pna.py:243-245);
 * src / dst: the edge list in the order of the rows of `out` (the kernels' destination-sorted order).  take_sqrt: the distance
 * itself, torch.norm(x_src - x_dst, dim=-1) - PNATower.pretrans_edges with use_3d=True (reference models/pna_original.py:224-226) */
int i3d_edge_sqdist(const float* x, const int* src, const int* dst, int num_edges, float* out, int ld, int col, int take_sqrt,
                    void* stream);

/* ---- one PNALayer of the tower variant from ONE call per direction (csrc/tower.hip) --------------------------------------
 * Replaces PNALayer.forward of reference models/pna_original.py:296-319 (all `towers` PNATower.forward, :239-261, the
 * concatenation, the mixing network, LeakyReLU and the residual) and its autograd backward, on the STACKED form of the
 * towers: Wp [f_msg, 2 f_in + f_edge] (pitch ldp) = every tower's pretrans Linear, Wq [f_out, f_in + B f_msg] (pitch ldq) =
 * every tower's posttrans Linear (B = n_aggregators * n_scalers column blocks of f_msg), bq / gamma / beta / running
 * statistics [f_out] side by side, Wm [f_mix, f_out] / bm the mixing network.  h [N, f_in], e [E, f_edge] (destination-
 * sorted, or NULL), snorm [N] or NULL (graph norm), out [N, f_mix]; residual needs f_mix == f_in.  gamma NULL: no BatchNorm.
 * saved / scratch: i3d_tower_layer_saved_floats / _scratch_floats floats (the forward's `saved` is the backward's).
 * workspace: i3d_colreduce_workspace_bytes, zero-initialised; gemm_workspace: the split-K scratch of the weight gradients.
 * Backward: grad_out [N, f_mix] -> grad_h [N, f_in] (written), grad_e [E, f_edge] (written, or added to when
 * grad_e_accumulate; NULL: not wanted), parameter gradients (grad_Wp / grad_Wq with pitches ldgp / ldgq). */
typedef struct {
    int num_nodes, num_edges, f_in, f_edge, f_msg, f_out, f_mix, ldp, ldq, ldgp, ldgq;
    int n_aggregators, n_scalers, residual, training, grad_e_accumulate;
    int aggregators[8], scalers[4];
    float avg_d_log, eps, momentum;
    const float* h;
    const float* e;
    const float* snorm;
    const float* Wp;
    const float* bp;
    const float* Wq;
    const float* bq;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    const float* Wm;
    const float* bm;
    const int* src_s;
    const int* dst_s;
    const int* in_ptr;
    const int* out_ptr;
    const int* out_epos;
    float* saved;
    float* scratch;
    void* workspace;
    void* gemm_workspace;
    long gemm_workspace_bytes;
    float* out;
    const float* grad_out;
    float* grad_h;
    float* grad_e;
    float* grad_Wp;
    float* grad_bp;
    float* grad_Wq;
    float* grad_bq;
    float* grad_gamma;
    float* grad_beta;
    float* grad_Wm;
    float* grad_bm;
    /* > 1: the posttrans products as n_towers diagonal blocks (i3d_gemm_f32_batched) - tower t's rows of Wq hold its f_msg / n_towers
     * x B aggregated columns at f_in + t B f_msg / n_towers .. (zeros elsewhere are never read) and the aggregation is written /
     * its gradient read tower-major (i3d_pna_aggregate_fwd_towers); needs f_msg / n_towers and f_out / n_towers multiples of 4.
     * 0 / 1: one dense product on [block][tower][feature] columns */
    int n_towers;
    /* > 0: the scalers folded into per-degree weights as in the 2D network's posttrans block (above:
     * "degree-grouped posttrans") - the aggregation writes its identity blocks only ([N, n_aggregators f_msg]), the product on it
     * is grouped by in-degree with W_D = sum_s coef[g][s] W_s: K of the dominant products n_scalers times shorter, the aggregated
     * tensor n_scalers times smaller.  group_start / group_count / coef / deg_rows / deg_tile_group / m_padded as in
     * I3dGroupedFcArgs (graph.py: GraphIndex.degree_groups).  With n_towers > 1 as well: the columns behind f_in are
     * [scaler][tower][aggregator][feature], the aggregation is written tower-major and the per-degree weights' diagonal blocks
     * are multiplied (i3d_gemm_f32_grouped_batched); the weight gradient stays one dense grouped product */
    int n_deg_groups, m_padded;
    int group_start[32];
    int group_count[32];
    float coef[128];
    const int* deg_rows;
    const int* deg_tile_group;
} I3dTowerLayerArgs;
long i3d_tower_layer_saved_floats(const I3dTowerLayerArgs* a);
long i3d_tower_layer_scratch_floats(const I3dTowerLayerArgs* a);
int i3d_tower_layer_fwd(const I3dTowerLayerArgs* a, void* stream);
int i3d_tower_layer_bwd(const I3dTowerLayerArgs* a, void* stream);

/* ---- BatchNorm out of the memory path (csrc/fused_bn.hip, csrc/gemm.hip; reference models/base_layers.py:100-111) ----
 * Column statistics as per-row-tile partials  partial[tile][3][feat] = {sum, M2 about the tile mean, row count},
 * produced by the kernel that writes the activation; i3d_bn_finalize_partials merges them (fp64, fixed order) into
 * mean / invstd / running statistics (momentum, unbiased running_var, num_batches_tracked += 1) and
 * aff[3 feat] = mean | gamma * invstd | beta, which the CONSUMER of the activation applies while loading it. */
int i3d_bn_finalize_partials(const float* partial, int n_tiles, int feat, float eps, float momentum, const float* gamma,
                             const float* beta, float* mean, float* invstd, float* running_mean, float* running_var,
                             long long* num_batches_tracked, float* aff, void* stream);
/* x[j,:] = act(P[src_s[j], 0:feat] + P[dst_s[j], feat:2 feat] + Q[q_code ? q_code[j] : j, :] + bias) and the partials of x;
 * a tile is i3d_edge_stats_rows_per_tile(feat) consecutive rows (reference models/pna.py:237-252 + base_layers.py:102-108) */
int i3d_edge_stats_rows_per_tile(int feat);
int i3d_edge_combine_act_stats(const float* P, int ldp, const float* Q, const int* q_code, const float* bias,
                               const int* src_s, const int* dst_s, int num_edges, int feat, int act, float* x,
                               float* partial, void* stream);
/* C[M,N] = epi_act(A' W^T + bias (+ C)),  A' = (A - mean) * scale + shift per column k when a_aff ([3K]) is given (the
 * BatchNorm of the block in front applied while A is staged), W [N,K] row-major; stats ([ceil(M/64)][3][N]) receives the
 * partials of the stored values per 64-row tile.  Grouped form as i3d_gemm_f32_grouped (m_rows padded to 64 per group with
 * -1, M = padded count, a_rows_total = physical rows of A / C).  Needs 16-byte aligned operands, K % 4 == 0.  epi_act: none, ReLU
 * or LeakyReLU (the activations of the blocks this product sits in; any other runs as a pass of its own behind a plain product). */
int i3d_gemm_f32_fused(int M, int N, int K, const float* A, int lda, long a_rows_total, const float* W, int ldb, float* C,
                       int ldc, const float* bias, int accumulate, const float* a_aff, int epi_act, float* stats,
                       const int* m_rows, const int* tile_group, long b_group_stride, void* stream);
/* i3d_gemm_f32_fused whose `accumulate` addend is read from c_in (row pitch ldcin) instead of C */
int i3d_gemm_f32_fused_src(int M, int N, int K, const float* A, int lda, long a_rows_total, const float* W, int ldb, float* C,
                           int ldc, const float* c_in, int ldcin, const float* bias, int accumulate, const float* a_aff,
                           int epi_act, float* stats, const int* m_rows, const int* tile_group, long b_group_stride,
                           void* stream);
/* i3d_gemm_f32_fused (statistics variant) with the output stored as bf16 - row r at (bf16*)C + r * ldc, rounded where it is
 * stored, statistics from the fp32 values (the bf16 matmul mode's storage form of a PNA layer's messages) */
int i3d_gemm_f32_fused_bf16out(int M, int N, int K, const float* A, int lda, long a_rows_total, const float* W, int ldb, void* C, int ldc,
                               const float* bias, const float* a_aff, int epi_act, float* stats, void* stream);
/* Wcat [2 f_out_edge + f_out_post, f_h] = [W_s ; W_d ; W_h], bcat = [0 | 0 | bias_post] (I3dPnaLayerArgs.merge_h) */
int i3d_pna_pack_h_weights(const float* W_edge, int ldw_edge, int f_out_edge, const float* W_post, int ldw_post, int f_out_post,
                           const float* bias_post, int f_h, float* Wcat, float* bcat, void* stream);
/* i3d_bn_bwd (local statistics or the process-wide collectives) with grad_pre as a column block of a wider
 * matrix: row pitch ld_out floats */
int i3d_bn_bwd_strided(const float* grad_y, const float* x, const float* pre, int rows, int feat, int act, int post_act,
                       const float* mean, const float* invstd, const float* gamma, const float* beta, float* grad_gamma,
                       float* grad_beta, float* grad_pre, int ld_out, float* grad_bias, void* workspace, void* stream);
/* i3d_bn_bwd with the BatchNorm input x stored as bf16 (row r at (bf16*)x + r * feat) */
int i3d_bn_bwd_x_bf16(const float* grad_y, const void* x, int rows, int feat, int act, int post_act, const float* mean,
                      const float* invstd, const float* gamma, const float* beta, float* grad_gamma, float* grad_beta, float* grad_pre,
                      float* grad_bias, void* workspace, void* stream);
/* dW[f_out,f_in] = dY^T y for y = (x - mean) * scale + shift (aff over f_in) computed from the raw x; grad_bias[f_out] =
 * column sums of dY (already computed) */
int i3d_gemm_f32_wgrad_bn(int f_out, int f_in, int rows, const float* dY, int ldy, const float* x, int ldx, float* dW,
                          int ldw, const float* grad_bias, const float* aff, void* workspace, long workspace_bytes,
                          void* stream);
/* ---- synchronised BatchNorm from inside the sequencers: process-wide collectives (csrc/comm.hip) ---------------------
 * The reference's BatchNorm statistics are over the whole batch (models/base_layers.py:87, 100-111); with the batch
 * sharded over ranks, i3d_bn_finalize_partials, i3d_act_stats_fwd[_counted] (sums_out NULL) and i3d_bn_bwd
 * (sums_out / sums_in NULL) synchronise their statistics over the ranks WHILE a collective table is set: local merge ->
 * collective on the caller's stream -> finalisation over all ranks (running statistics = global, grad_gamma / grad_beta =
 * this rank's share: the gradient all-reduce sums them).  world 1 runs the same sequence (self-test).
 *   all_gather_f32: recv[world][count] <- every rank's send[count];  all_reduce_f64: buf[count] summed in place
 *   scratch: device memory of the table's own (>= (4 + 3 world) * widest BatchNorm * 8 bytes; 1 MiB is plenty)
 * Providers: callbacks (i3d_set_collectives), RCCL (below), peer-write exchange (further below: the production one).
 * RCCL provider: rank 0 i3d_rccl_unique_id -> (caller broadcasts the 128 bytes) -> every rank i3d_rccl_init ->
 * i3d_set_collectives_rccl.  i3d_set_collectives(NULL): off.  One training per process. */
typedef struct {
    int world;
    int (*all_gather_f32)(void* user, const float* send, float* recv, long count, void* stream);
    int (*all_reduce_f64)(void* user, double* buf, long count, void* stream);
    void* user;
    void* scratch;
    long scratch_bytes;
} I3dCollectives;
int i3d_set_collectives(const I3dCollectives* c /* host; copied */);
int i3d_collectives_world(void); /* 0: none set */
/* The installed provider's collectives as the BatchNorm entry points call them when no fused exchange applies: recv[world][count]
 * <- every rank's send[count]; buf[count] <- sum over the ranks (the peer provider: in rank order).  The vectors are staged through the
 * table's scratch as the BatchNorm entry points stage theirs ((count + world count) floats / count doubles must fit).  For a binding's
 * self-test (tests/test_gpu_dist.py); every rank makes the same calls in the same order on one stream.  (No reference counterpart:
 * SURVEY.md C3.) */
int i3d_collectives_all_gather_f32(const float* send, float* recv, long count, void* stream);
int i3d_collectives_all_reduce_f64(double* buf, long count, void* stream);
int i3d_rccl_available(void);
int i3d_rccl_unique_id(char* out128 /* host */);
int i3d_rccl_init(const char* id128 /* host */, int rank, int world, void** comm);
int i3d_rccl_destroy(void* comm);
int i3d_set_collectives_rccl(void* comm, int world, void* scratch, long scratch_bytes);
/* ---- provider 3: one-shot peer-write exchange over IPC-mapped mailboxes (csrc/peer.h, peer.hip) -----------------------
 * What the reference's whole-batch BatchNorm (models/base_layers.py:87, 100-111: nn.BatchNorm1d over every row the model is
 * given) costs once the batch is sharded over ranks: ~50 vectors of <= [3F] floats per step, each needed by every rank, on
 * the step's dependent chain.  Every rank allocates a mailbox (i3d_peer_alloc: uncached device memory + its IPC handle),
 * the caller distributes the handles (torch.distributed all_gather_object), every rank maps the others' mailboxes
 * (i3d_peer_open) and installs the provider (i3d_set_collectives_peer).  While it is installed
 *   - i3d_bn_finalize_partials exchanges its {sum, M2, count} triples INSIDE the finalisation kernel (one launch, as
 *     without synchronisation);
 *   - i3d_bn_bwd*, i3d_act_stats_fwd* and the 3D network's edge stage exchange their fp64 sums in one launch
 *     (append row count -> sum over ranks in rank order -> fp32 vectors + 1 / rows);
 *   - the table's generic all_gather_f32 / all_reduce_f64 are one-launch kernels of the same protocol.
 * A kernel writes payload + sequence flag into every rank's mailbox and waits (bounded: timeout_s, default 30 s,
 * I3D_PEER_TIMEOUT_S) for the `world` flags in its own; a wait that times out is reported by the NEXT call (error return,
 * i3d_peer_status) - no hung GPU.  One stream issues the collectives, in the same order on every rank.  Results are
 * bit-identical on all ranks (sums in rank order).  world <= 16, BatchNorm width <= 4095. */
long i3d_peer_mailbox_bytes(void);
int i3d_peer_handle_bytes(void); /* sizeof(hipIpcMemHandle_t) = 64 */
int i3d_peer_alloc(void** mailbox /* out: device */, char* handle_out /* host, i3d_peer_handle_bytes() */);
int i3d_peer_free(void* mailbox); /* a mailbox that did not end up in a context (i3d_peer_close frees the one it owns) */
int i3d_peer_open(void* mailbox, const char* handles /* host [world][handle bytes], rank order */, int rank, int world,
                  double timeout_s /* <= 0: default */, void** ctx /* out */);
int i3d_set_collectives_peer(void* ctx, void* scratch, long scratch_bytes);
/* a second context (own mailbox, sequence and scratch) for the collectives issued on `stream`: the 3D network's side stream keeps
 * running beside the 2D network under synchronised BatchNorm; every rank binds the same streams in the same roles */
int i3d_peer_bind_stream(void* ctx, void* stream, void* scratch, long scratch_bytes);
int i3d_peer_status(void* ctx); /* 0: healthy, else the sequence number of the collective whose wait timed out */
long long i3d_peer_sequence(void* ctx); /* collectives issued so far */
int i3d_peer_close(void* ctx); /* unmaps the peers, frees the mailbox; every rank must have stopped issuing collectives */

/* ---- all weight gradients of a layer in ONE launch + one fixed-order reduction (csrc/wgrad.hip) ----------------------
 * Replaces autograd's dW = dY^T X of every nn.Linear of a PNA layer (reference models/base_layers.py:101; the Linears of
 * models/pna.py:186-197) - round 2 issued them as ~10 launches per layer.  A problem is one product
 *     P[M,N] = sum_{k_begin <= k < k_begin + k_count} A[row(k), 0:M]^T B[row(k), 0:N],   row(k) = rows ? rows[k] : k
 * (rows[k] = -1: padding, contributes nothing; rows_total = physical rows of A and B).  An output takes the products of
 * n_groups consecutive problems (first_problem ...), all of one shape:
 *   I3D_WGRAD_PLAIN   (n_groups 1)  C[m, n] = P, rows m >= c_split displaced by c_delta floats (c_split 0: none)
 *   I3D_WGRAD_BN      (n_groups 1)  C = (P - row[m] mean[n]) scale[n] + row[m] shift[n], aff = mean | scale | shift [3N]:
 *                     the product against a BatchNorm output that was never materialised (i3d_gemm_f32_wgrad_bn)
 *   I3D_WGRAD_COMBINE               C[m, s * scaler_stride + n] = sum_g coef[g * n_scalers + s] P_g  (host coef): the
 *                     per-degree posttrans gradients folded into the scaler blocks (i3d_pna_combine_weights_bwd); at
 *                     most one such output per call
 * Needs M, N, lda, ldb, ldc multiples of 4 and 16-byte aligned pointers (i3d_wgrad_multi_supported), and
 * i3d_wgrad_multi_workspace_bytes(units) of scratch for `units` K-slice panels (more scratch = shorter slices, up to
 * I3D_WGRAD_UNITS = 256 by default).  Deterministic: every slice is summed in a fixed order. */
#define I3D_WGRAD_PLAIN 0
#define I3D_WGRAD_BN 1
#define I3D_WGRAD_COMBINE 2
typedef struct {
    const float* A;
    const float* B;
    const int* rows;
    long rows_total;
    int lda, ldb, M, N;
    int k_begin, k_count;
} I3dWgradProblem;
typedef struct {
    int kind, n_groups, first_problem;
    int ldc, c_split, n_scalers;
    long c_delta, scaler_stride;
    float* C;
    const float* aff;
    const float* row;
    const float* coef; /* host */
} I3dWgradOutput;
int i3d_wgrad_multi_supported(const I3dWgradProblem* problems, int n_problems, const I3dWgradOutput* outputs, int n_outputs);
long i3d_wgrad_multi_workspace_bytes(int max_units);
long i3d_wgrad_multi_min_workspace_bytes(const I3dWgradProblem* problems, int n_problems); /* with the longest slices */
int i3d_wgrad_multi(const I3dWgradProblem* problems, int n_problems, const I3dWgradOutput* outputs, int n_outputs,
                    void* workspace, long workspace_bytes, void* stream);

/* i3d_pna_aggregate_fwd / _bwd with the messages read as (e - mean) * scale + shift (aff [3 feat], may be NULL).  A non-NULL aff
 * needs feat % 4 == 0 and a 16-byte aligned aff (the kernels load it in 16-byte items): BOTH directions, and their _ex forms,
 * return I3D_ERR_INVALID otherwise, before any launch.  The gradient is the one with respect to the normalised message. */
int i3d_pna_aggregate_fwd_aff(const float* e, const float* aff, const int* in_ptr, int num_nodes, int feat,
                              const int* aggregators, int n_aggregators, const int* scalers, int n_scalers,
                              int force_scalers, float avg_d_log, float* out, void* stream);
int i3d_pna_aggregate_bwd_aff(const float* grad_out, const float* e, const float* aff, const int* in_ptr, int num_nodes,
                              int feat, const int* aggregators, int n_aggregators, const int* scalers, int n_scalers,
                              int force_scalers, float avg_d_log, float* grad_e, void* stream);
/* the same two with the messages stored as bf16 (e_bf16 != 0: row r of the [E, feat] message matrix at (bf16*)e + r * feat, feat a
 * multiple of 4, 8-byte aligned; the bf16 matmul mode's storage form of the last pretrans block's activation): K4 reads half the
 * message bytes; outputs and gradients stay fp32 */
int i3d_pna_aggregate_fwd_ex(const void* e, int e_bf16, const float* aff, const int* in_ptr, int num_nodes, int feat,
                             const int* aggregators, int n_aggregators, const int* scalers, int n_scalers, int force_scalers,
                             float avg_d_log, float* out, void* stream);
int i3d_pna_aggregate_bwd_ex(const float* grad_out, const void* e, int e_bf16, const float* aff, const int* in_ptr, int num_nodes,
                             int feat, const int* aggregators, int n_aggregators, const int* scalers, int n_scalers,
                             int force_scalers, float avg_d_log, float* grad_e, void* stream);

/* The BatchNorm backward (i3d_bn_bwd and its variants; reference models/base_layers.py:100-111 under autograd) as ONE launch for
 * tensors of up to 256 * (2048 / feat) * 8 rows, feat % 4 == 0, feat <= 2048, activations none / ReLU / LeakyReLU: a workgroup
 * keeps its row chunk in registers across an in-launch reduction (every workgroup of the launch is resident: <= 256 workgroups,
 * two per CU).  Process-wide, on by default (environment I3D_BN_BWD_ONE_LAUNCH=0); switch it OFF when several processes share
 * one GPU (their launches compete for the CUs and the residency argument no longer holds).  Returns the previous setting. */
int i3d_set_bn_bwd_one_launch(int on);
int i3d_bn_bwd_one_launch_supported(int rows, int feat); /* 1: a local (not synchronised) i3d_bn_bwd of this shape takes it */
long i3d_bn_bias_partial_floats(int feat); /* floats of the partials buffer i3d_colsum_strided takes */
/* The BatchNorm backward of a PNA layer's edge block (the FCLayer inside pretrans_edges, reference models/pna.py:237-252 with
 * models/base_layers.py:100-111) fused with the two segmented sums behind it: column sums of dy and dy xhat as i3d_bn_bwd (one
 * launch; grad_gamma / grad_beta), then ONE launch that forms the data gradient g of every edge row inside the sums that consume
 * it - out_src[v] = sum of g over the out-edges of v (rows out_epos[out_ptr[v] .. out_ptr[v+1])), out_dst[v] = sum over its
 * in-edges (rows in_ptr[v] .. in_ptr[v+1]) - and stores g to grad_pre [rows, feat].  The same bits as i3d_bn_bwd followed by
 * i3d_segment_sum_pair.  act: none / ReLU / LeakyReLU; feat % 4 == 0, feat <= 512; synchronised statistics as i3d_bn_bwd.
 * The bias gradient of the Linear in front is the column sum of out_dst: i3d_colsum_strided (any stream). */
int i3d_bn_bwd_edge_sums(const float* grad_y, const float* x, int rows, int feat, int act, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float* grad_gamma, float* grad_beta, float* grad_pre,
                         const int* in_ptr, const int* out_ptr, const int* out_epos, int num_nodes, float* out_src, float* out_dst,
                         int ldo, void* workspace, void* stream);
/* out[c] = sum over rows of x[r * ldx + c] (two launches, fixed order: deterministic); partial: i3d_bn_bias_partial_floats(feat) floats
 * of the caller's (the reduction's row-chunk partials - not the BatchNorm workspace, which another stream may be using) */
int i3d_colsum_strided(const float* x, int ldx, int rows, int feat, float* out, float* partial, void* stream);

/* ---- composites: one call enqueues a whole FCLayer-shaped block (forward or backward) ------------------------
 * "input operator -> Linear -> activation -> BatchNorm1d (training, local statistics) -> post-activation (+ residual)",
 * reference models/base_layers.py:100-111, with the three input operators of the PNA / Net3D layers.  Same kernels
 * as the per-kernel entry points above, sequenced in C++ so the host pays one transition per block instead of ~7-13.
 * All pointers are device pointers except the struct itself (host).  Forward fills xact (activation output, saved),
 * pre_keep (Linear output, only when the activation needs it: SiLU/Sigmoid; NULL otherwise: activation in place),
 * tail.mean / tail.invstd, y.  Backward reads them and fills the grad_* members (grad_x / grad_q may be NULL). */
typedef struct {
    int act, post_act;
    float eps, momentum;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* mean;
    float* invstd;
    void* workspace; /* i3d_colreduce_workspace_bytes(rows, f_out) */
    void* gemm_workspace; /* scratch of the weight-gradient GEMMs of the backward (i3d_gemm_f32_ws), may be NULL */
    long gemm_workspace_bytes;
    long long* num_batches_tracked; /* BatchNorm1d's int64 counter, incremented by the forward (may be NULL) */
} I3dBnTail;

typedef struct { /* y = tail(x W^T + b) */
    I3dBnTail tail;
    int rows, f_in, f_out, ldw;
    const float* x;
    const float* W;
    const float* bias;
    const float* residual;
    float* xact;
    float* pre_keep;
    float* y;
    const float* grad_y;
    float* grad_pre; /* scratch [rows, f_out] */
    float* grad_gamma;
    float* grad_beta;
    float* grad_W;
    float* grad_bias;
    float* grad_x;
    void* W_dgrad_panel; /* optional: the block's weight packed for the row-panel data gradient (i3d_panel_pack(W, ldw, f_in, f_out,
                          * trans 0): i3d_panel_packed_bytes(f_in, f_out) bytes) - filled by i3d_pna_layer_weights_fwd / the layer's
                          * forward pass, read by its backward pass (dX = dZ W through i3d_panel_gemm).  NULL: the tiled product */
    void* W_fwd_panel;   /* optional: the same weight packed for the row-panel FORWARD product of the fused-BatchNorm layer path
                          * (i3d_panel_pack(W, ldw, f_out, f_in, trans 1): i3d_panel_packed_bytes(f_out, f_in) bytes) */
} I3dFcArgs;

typedef struct { /* y = tail(P[src,:F] + P[dst,F:] + q W_q^T + b),  P = h [W_s|W_d]^T  (reference models/pna.py:237-252) */
    I3dBnTail tail;
    int num_nodes, num_edges, f_h, f_q, f_out, ldw;
    int q_rows;  /* 0: q is [E, f_q];  V > 0: q is the [V, f_q] table of all categorical combinations (i3d_edge_codes) */
    int v_pad;   /* leading dimension of onehot */
    const int* q_code;   /* [E] row of q for every edge (table mode) */
    const float* onehot; /* [E, v_pad] */
    float* grad_Q;       /* scratch [v_pad, f_out] (table mode) */
    const float* h;
    const float* q;
    const float* W;
    const float* bias;
    const int* src_s;
    const int* dst_s;
    const int* in_ptr;
    const int* out_ptr;
    const int* out_epos;
    float* P; /* [N, 2*f_out] scratch */
    float* Q; /* [E, f_out] ([V, f_out] in table mode) scratch (NULL when q is NULL) */
    float* xact;
    float* pre_keep;
    float* y;
    const float* grad_y;
    float* grad_pre; /* scratch [E, f_out] */
    float* grad_P;   /* scratch [N, 2*f_out] */
    float* grad_gamma;
    float* grad_beta;
    float* grad_W;
    float* grad_bias;
    float* grad_h;
    float* grad_q;
    int grad_q_accumulate; /* grad_q += ... instead of = (a q shared by several layers: the bond table) */
} I3dEdgeFcArgs;

typedef struct { /* y = tail(h W_h^T + b + agg[deg group] W_D^T),  W_D = sum_s coef[g][s] W_s  (models/pna.py:207-209, 229-233) */
    I3dBnTail tail;
    int num_nodes, f_h, f_out, agg_width, ldw, n_groups, n_scalers, m_padded;
    int group_start[32];
    int group_count[32];
    float coef[128]; /* [n_groups][n_scalers] */
    const float* h;
    const float* agg;
    const float* W;
    const float* bias;
    const float* residual;
    const int* deg_rows;
    const int* deg_tile_group;
    float* WD; /* [n_groups, f_out, agg_width] */
    float* xact;
    float* pre_keep;
    float* y;
    const float* grad_y;
    float* grad_pre; /* scratch [N, f_out] */
    float* grad_WD;  /* scratch like WD */
    float* grad_gamma;
    float* grad_beta;
    float* grad_W;
    float* grad_bias;
    float* grad_h;
    float* grad_agg;
} I3dGroupedFcArgs;

#define I3D_MAX_EXTRA_FC 3
typedef struct { /* one PNA layer, reference models/pna.py:199-216: pretrans edge MLP (edge block + n_pre_extra plain FC
                  * blocks) -> aggregation (i3d_pna_aggregate_*) -> posttrans (degree-grouped block + n_post_extra plain FC
                  * blocks) + residual.  The member blocks are chained by the caller (pre[0].x = edge.y, ...); forward
                  * and backward are the member composites back to back, the three contributions to dL/dh (posttrans,
                  * edge MLP, residual) are summed into post.grad_h. */
    I3dEdgeFcArgs edge;
    int n_pre_extra;
    I3dFcArgs pre[I3D_MAX_EXTRA_FC];
    int n_aggregators, n_scalers, force_scalers;
    int aggregators[8];
    int scalers[4];
    float avg_d_log;
    const float* msg;      /* [E, F] output of the pretrans MLP (= y of its last block) */
    float* grad_msg;       /* [E, F] scratch: gradient of the messages */
    I3dGroupedFcArgs post;
    int n_post_extra;
    I3dFcArgs postx[I3D_MAX_EXTRA_FC];
    int residual;          /* h_new += h (fused into the last block's BN apply by the caller via its residual pointer) */
    const float* grad_out; /* [N, F] incoming gradient of the layer output (added to post.grad_h when residual) */
    void* agg_event_start; /* optional (i3d_event_create): recorded on the stream right before / after the forward */
    void* agg_event_stop;  /* aggregation kernel - the roofline measurement of bench.py */
    /* fused BatchNorm (csrc/fused_bn.hip): statistics out of the producers' epilogues, BatchNorm-apply in the consumers'
     * loads.  Then edge.y / pre[i].y are not written (may be NULL), msg = the xact of the last pretrans block, and the
     * degree groups of `post` must cover every node (in-degree 0 included, zero coefficients).  Needs activations whose
     * derivative follows from the output (none / ReLU / LeakyReLU), no post-activation, n_post_extra == 0. */
    int fused_bn;
    int defer_join; /* backward: do not wait for the weight-gradient stream at the end of the layer; the caller keeps every
                     * buffer that stream reads or writes alive and calls i3d_wgrad_stream_join before it consumes them */
    float* stats_ws;                   /* scratch, i3d_pna_layer_stats_floats(...) floats */
    float* aff[I3D_MAX_EXTRA_FC + 1];  /* [3 f_out] mean | gamma invstd | beta of the edge block and of pre[i] (saved) */
    int weights_ready; /* forward (fused_bn): edge.Q and post.WD - products of parameters and the bond table only - are already
                        * there (i3d_pna_layer_weights_fwd, e.g. on the side stream while the layers before this one run) */
    /* round 3: the products that read the node features h as ONE GEMM per direction.  Forward: PL [N, 2 f_out(edge) + f_out(post)]
     * = h Wcat^T + bcat (Wcat = [W_s ; W_d ; W_h] packed by i3d_pna_pack_h_weights) - its first 2 f_out columns are the edge
     * block's P, the rest the posttrans block's h-product, which the grouped GEMM takes as its addend.  Backward: DL (same
     * shape) = [dP | dlin], dL/dh (+)= DL Wcat in one GEMM at the end of the layer.  merge_h = 1 needs fused_bn,
     * n_post_extra == 0 and the four buffers (Wcat, bcat, PL saved by the forward pass; DL backward scratch that the
     * weight-gradient stream reads). */
    int merge_h;
    float* Wcat;
    float* bcat;
    float* PL;
    float* DL;
    int wgrad_split;   /* backward: issue the posttrans weight gradients as soon as the posttrans chain is done and the rest at the
                        * end, as two launches (the last layer of a backward pass: nothing runs next to its weight gradients
                        * once the chain has ended); 0: one launch at the end of the layer */
    int eval_mode;     /* forward (fused_bn) in eval(): BatchNorm with the running statistics (reference: nn.BatchNorm1d in eval
                        * mode, trainer/trainer.py:75 model.eval()) - aff[i] already hold mean | gamma / sqrt(var + eps) | beta
                        * (i3d_bn_eval_aff_multi), no statistics are finalised, no running statistic is touched */
    int msg_bf16;      /* fused_bn with at least one later pretrans block, bf16 matmul mode: `msg` (= the last pretrans block's xact,
                        * [E, f_msg]) holds bf16 - written by that block's GEMM epilogue, read by the aggregation kernels and by the
                        * block's BatchNorm backward; the buffer keeps its fp32 size.  Same value forward and backward. */
    float* edge_bias_partial; /* backward, optional (i3d_bn_bias_partial_floats(edge.f_out) floats): with it (and merge_h, an
                        * activation of the none / ReLU / LeakyReLU class, 16-byte rows) the edge block's BatchNorm backward runs
                        * as i3d_bn_bwd_edge_sums - the data gradient formed inside the two segmented sums behind it - and its
                        * bias gradient is taken from dP[dst] on the weight-gradient stream through this buffer */
    void* Wcat_panel;  /* optional (merge_h): Wcat packed for the row-panel forward product PL = h Wcat^T + bcat (i3d_panel_pack, trans 1:
                        * i3d_panel_packed_bytes(2 f_out(edge) + f_out(post), f_h) bytes), packed where Wcat is.  NULL: the tiled product */
    void* Wcat_dgrad_panel; /* optional (merge_h): Wcat packed for the backward product dL/dh (+)= DL Wcat (trans 0:
                        * i3d_panel_packed_bytes(f_h, 2 f_out(edge) + f_out(post)) bytes) */
} I3dPnaLayerArgs;

/* eval-mode affine vector of one BatchNorm: aff [3 feat] = running_mean | gamma / sqrt(running_var + eps) | beta */
typedef struct {
    const float* running_mean;
    const float* running_var;
    const float* gamma;
    const float* beta;
    float* aff;
    int feat;
    float eps;
} I3dBnEvalAff;
int i3d_bn_eval_aff_multi(const I3dBnEvalAff* entries /* host */, int n, void* stream);

/* floats of I3dPnaLayerArgs.stats_ws for a layer with these dimensions (f = widest block output) */
long i3d_pna_layer_stats_floats(int num_nodes, int num_edges, int m_padded, int f);

/* Where the buffers of one PNA layer live: the ONE list of a layer's saved and scratch buffers, for every sequencer.
 * The caller describes the layer - the sizes of every block and ldw, n_pre_extra / n_post_extra / n_aggregators, each tail's
 * act / post_act, fused_bn, merge_h, whether there is a q (edge.f_q > 0; a placing call wants edge.q itself then) / q_rows /
 * v_pad, post.n_groups / agg_width (backward also: grad_out) - and these fill in every saved or scratch pointer and chain
 * the blocks (pre[0].x = edge.y or, fused, edge.xact; msg; postx[0].x = post.y; backward: each block's grad_y = the grad_x
 * of the block behind it, the top one = grad_out).  A buffer the
 * description rules out (pre_keep under none / ReLU / LeakyReLU, y of a fused pretrans block, aff[] of a non-fused one, the
 * merge_h buffers and panel images without merge_h, Q / grad_Q without q or a table) is set to NULL.  Left to the caller:
 * h, q, parameters and their gradients, index arrays, stats_ws, the layer output (y of the last posttrans block) and the
 * residual pointers, grad_out, post.grad_h, edge.grad_q / grad_q_accumulate, workspaces, events, control flags.
 * Every buffer starts a multiple of 4 floats from its base.  A NULL base: sizing only (the pointers come out NULL).
 * Forward: returns the floats used behind `base`, < 0 for a description no layer has. */
long i3d_pna_layer_place_fwd(I3dPnaLayerArgs* args, float* base);
/* Backward: `chain` takes the buffers only the layer's own stream touches (a sequencer may reuse it layer by layer), `side`
 * those the weight-gradient stream reads or writes (alive until that stream is joined).  Both counts are always written. */
int i3d_pna_layer_place_bwd(I3dPnaLayerArgs* args, float* chain, float* side, long* chain_floats, long* side_floats);

/* ---- the edge stage of the 3D network, one lane per edge (net3d_edge.hip) ---------------------------------------
 * reference models/net3d.py:57-81 + 100-118 for propagation_depth 1, one message block, broadcast node embedding:
 *   e0 = post(BN_in(act(W_in fourier(d) + b_in))),  m = BN_msg(act(W_msg [emb | emb | e0] + b_msg)),
 *   m_sum[v] = mean/sum over the in-edges of m * sigmoid(w_gate . m + b_gate)
 * Forward fills d_out (e0 in edge-id order: what the reference leaves in graph.edata['d']), x_msg, aff_*, tail_*.mean /
 * invstd (running statistics updated), m_sum.  Backward reads them and grad_m_sum and fills the grad_* members
 * (grad_emb is accumulated into: the caller has put the node-level part there). */
typedef struct {
    I3dBnTail tail_in;   /* edge-input block: act, post_act, BatchNorm over [E, hidden] (workspace members unused) */
    I3dBnTail tail_msg;  /* message block: act, BatchNorm (post_act must be none) */
    int num_nodes, num_edges, hidden, n_enc, reduce_mean;
    int ld_w_in, ld_w_msg;
    const float* d_raw;  /* [E] distances, edge-id order */
    const int* perm;     /* [E] edge id of the j-th edge in destination-sorted order */
    const int* dst_s;    /* [E] destination node, destination-sorted */
    const int* in_ptr;   /* [N + 1] */
    const float* emb;    /* [hidden] */
    const float* W_in;   /* [hidden, 2 n_enc + 1 (1 when n_enc == 0)] */
    const float* b_in;
    const float* W_msg;  /* [hidden, 3 hidden] */
    const float* b_msg;
    const float* w_gate; /* [hidden] */
    const float* b_gate; /* [1] */
    float* stats;        /* scratch, i3d_net3d_edge_stats_floats(E, hidden) floats */
    float* aff_in;       /* [3 hidden] saved */
    float* aff_msg;      /* [3 hidden] saved */
    float* x_msg;        /* [E, hidden] saved: activation output of the message block, destination-sorted */
    float* d_out;        /* [E, hidden] saved + graph side effect, edge-id order */
    float* msg;          /* [E, hidden] scratch (forward) */
    float* m_sum;        /* [N, hidden] out */
    const float* grad_m_sum; /* [N, hidden] */
    float* grad_ya;      /* scratch [E, hidden] (backward) */
    float* grad_lin;     /* unused since round 5 (the gradient of the message block's pre-activation stays in registers); may be null */
    float* partial;      /* scratch, i3d_net3d_edge_bwd_floats(E, hidden, n_enc) floats (backward) */
    float* grad_W_in;
    float* grad_b_in;
    float* grad_gamma_in;
    float* grad_beta_in;
    float* grad_W_msg;
    float* grad_b_msg;
    float* grad_gamma_msg;
    float* grad_beta_msg;
    float* grad_w_gate;
    float* grad_b_gate;
    float* grad_emb;     /* += */
    int store_bf16;      /* x_msg and msg - the [E, hidden] activations only this stage reads and writes - hold bf16 (the buffers
                          * keep their fp32 size): the bf16 matmul mode's storage form of the stage.  x_msg is stored about
                          * x_center (its columns can be nearly constant over a batch: see n3_center_kernel).  The same value in
                          * the forward and the backward call of a pass. */
    float* x_center;     /* [hidden] saved (store_bf16 only) */
} I3dNet3dEdgeArgs;
int i3d_net3d_edge_supported(int hidden, int n_enc);   /* 1 when the kernels are built for this combination */
long i3d_net3d_edge_stats_floats(int num_edges, int hidden);
long i3d_net3d_edge_bwd_floats(int num_edges, int hidden, int n_enc);
int i3d_net3d_edge_fwd(const I3dNet3dEdgeArgs* args, void* stream);
int i3d_net3d_edge_bwd(const I3dNet3dEdgeArgs* args, void* stream);

/* timing events for measurements around a kernel inside a composite (thin wrappers of hipEvent_t) */
int i3d_event_create(void** event);
int i3d_event_destroy(void* event);
int i3d_event_record(void* event, void* stream);
int i3d_event_elapsed_ms(void* start, void* stop, float* ms);   /* both events must have completed */

/* makes `stream` wait for everything its weight-gradient side stream holds (I3dPnaLayerArgs.defer_join) */
int i3d_wgrad_stream_join(void* stream);
/* the side stream of `stream`, ordered behind everything `stream` holds now (*side == stream when there is none) */
int i3d_wgrad_stream_fork(void* stream, void** side);
int i3d_wgrad_stream_peek(void* stream, void** side);      /* that stream without a new fork (`stream` itself if there is none) */
/* the parameter-only products of a fused_bn layer's forward: edge.Q = q W_q^T and post.WD = sum_s coef W_s */
int i3d_pna_layer_weights_fwd(const I3dPnaLayerArgs* args, void* stream);
int i3d_pna_layer_fwd(const I3dPnaLayerArgs* args, void* stream);
int i3d_pna_layer_bwd(const I3dPnaLayerArgs* args, void* stream);
int i3d_fc_bn_fwd(const I3dFcArgs* args, void* stream);
int i3d_fc_bn_bwd(const I3dFcArgs* args, void* stream);
/* the two halves of i3d_fc_bn_bwd: BatchNorm backward + data gradient (what the block in front waits for), and the weight
 * gradients (leaves: they may run on another stream that is ordered after the chain half, e.g. i3d_wgrad_stream_fork) */
int i3d_fc_bn_bwd_chain(const I3dFcArgs* args, void* stream);
int i3d_fc_bn_bwd_wgrad(const I3dFcArgs* args, void* stream);
int i3d_edge_fc_bn_fwd(const I3dEdgeFcArgs* args, void* stream);
int i3d_edge_fc_bn_bwd(const I3dEdgeFcArgs* args, void* stream);
int i3d_grouped_fc_bn_fwd(const I3dGroupedFcArgs* args, void* stream);
int i3d_grouped_fc_bn_bwd(const I3dGroupedFcArgs* args, void* stream);

/* ---- whole-model sequencing (csrc/model.hip): the PNA forward / backward of a training step from one C call each ----
 * replaces PNA.forward -> PNAGNN.forward -> [PNALayer.forward]* -> readout -> head (reference models/pna.py:131-135,
 * 161-166, 199-213, 127-129) and its autograd backward for the pre-training configuration: every block Linear ->
 * activation (none / ReLU / LeakyReLU) -> BatchNorm1d in training mode with local statistics, >= 2 degree scalers
 * (degree-grouped posttrans), categorical bond features (bond table), one posttrans block.  The memory layout of the
 * saved activations and of the backward scratch is computed here (i3d_pna_model_saved_floats / _scratch_floats). */
#define I3D_MAX_LAYERS 16
#define I3D_MAX_HEAD_FC 4
typedef struct { /* one FCLayer: Linear + optional BatchNorm1d (reference models/base_layers.py:23-111) */
    const float* W;     /* [f_out, f_in] row-major, contiguous */
    const float* bias;
    const float* gamma; /* NULL: no BatchNorm */
    const float* beta;
    float* running_mean;
    float* running_var;
    long long* num_batches_tracked;
    float* grad_W; /* outputs of the backward pass (written, not accumulated) */
    float* grad_bias;
    float* grad_gamma;
    float* grad_beta;
    int f_in, f_out, act;
    float eps, momentum;
} I3dFcParams;

typedef struct {
    int training; /* 1: BatchNorm with batch statistics (running statistics updated); 0: eval mode, forward only (the
                   * validation pass of trainer/trainer.py:72-78) */
    int n_layers, hidden, n_pre, residual;
    int n_aggregators, aggregators[8];
    int n_scalers, scalers[4];
    float avg_d_log;
    I3dFcParams pre[I3D_MAX_LAYERS][I3D_MAX_EXTRA_FC + 1]; /* pretrans blocks (block 0: [h_src | h_dst | e] -> f_out) */
    I3dFcParams post[I3D_MAX_LAYERS];                      /* posttrans block ([h | agg x scalers] -> hidden) */
    int n_atom_tables, atom_dims[16];
    const float* atom_tables[16];
    float* grad_atom_tables; /* [sum atom_dims, hidden]: the table gradients, contiguous in table order */
    int n_bond_tables, bond_dims[16];
    const float* bond_tables[16];
    float* grad_bond_tables;
    int n_readout, readout_ops[4];
    int n_head;
    I3dFcParams head[I3D_MAX_HEAD_FC];
} I3dPnaModel;

typedef struct {
    int num_nodes, num_edges, num_graphs;
    const int64_t* atom_feat; /* [N, n_atom_tables] */
    const int64_t* bond_feat; /* [E, n_bond_tables], edge-id order */
    const int* in_ptr;        /* the destination-sorted index of 3dinfomax_amd/graph.py: GraphIndex */
    const int* perm;
    const int* src_s;
    const int* dst_s;
    const int* out_ptr;
    const int* out_epos;
    const int* graph_ptr;
    const int* deg_rows; /* nodes grouped by in-degree (0 included), groups padded to 64 with -1 */
    const int* deg_tile_group;
    int m_padded, n_groups;
    int group_degree[32], group_start[32], group_count[32];
    const int64_t* comb; /* [n_comb, n_bond_tables]: every combination of the categorical bond features (device) */
    int n_comb, v_pad;
} I3dPnaBatch;

long i3d_pna_model_saved_floats(const I3dPnaModel* model, const I3dPnaBatch* batch);   /* -1: not supported */
long i3d_pna_model_scratch_floats(const I3dPnaModel* model, const I3dPnaBatch* batch);
/* out [B, f_out of the last head block]; node_emb [N, hidden] (the graph's ndata['feat'] side effect); edge_emb [E, hidden]
 * or NULL (edata['feat'] side effect); agg_events: NULL or 2 * n_layers events recorded around the aggregation kernels;
 * *ctx_out: host-side context for i3d_pna_model_bwd (valid while `saved` is), freed with i3d_pna_model_ctx_free */
int i3d_pna_model_fwd(const I3dPnaModel* model, const I3dPnaBatch* batch, float* saved, float* node_emb, float* edge_emb,
                      float* out, void* bn_workspace, void* const* agg_events, void* stream, void** ctx_out);
/* grads_from: the same model with its grad_* members set (they are chosen at backward time), or NULL to use the forward's */
int i3d_pna_model_bwd(void* ctx, const I3dPnaModel* grads_from, const float* grad_out, float* scratch, void* bn_workspace,
                      void* gemm_workspace, long gemm_workspace_bytes, void* stream);
/* the backward pass in two calls (data parallel: the all-reduce of the first part's gradients runs next to the second):
 * part 1 = head + layers [split, n_layers), part 2 = layers [0, split) + encoders; part 0 = everything */
int i3d_pna_model_bwd_part(void* ctx, const I3dPnaModel* grads_from, const float* grad_out, float* scratch, void* bn_workspace,
                           void* gemm_workspace, long gemm_workspace_bytes, int part, int split, void* stream);
int i3d_pna_model_ctx_free(void* ctx);
/* test entries: out [rows, feat] = (e - mean) * scale + shift exactly as i3d_pna_aggregate_*_aff read the messages
 * (aff = mean | scale | shift, NULL: a copy); the messages of one layer of a forward pass from its context, [E, f_msg] in
 * destination-sorted order - the tests derive the kernels' arg-max / arg-min routing from them */
int i3d_pna_messages_normalized(const float* e, const float* aff, long rows, int feat, float* out, void* stream);
int i3d_pna_messages_normalized_ex(const void* e, int e_bf16, const float* aff, long rows, int feat, float* out, void* stream);
int i3d_pna_model_debug_messages(void* ctx, int layer, float* out, void* stream);

/* ---- Adam step of all parameter tensors in one launch (csrc/adam.hip; reference: torch.optim.Adam built by name,
 * train.py:189, stepped at trainer/trainer.py:120).  chunk_table: device array of n_chunks records {float* param,
 * const float* grad, float* exp_avg, float* exp_avg_sq, int n} (i3d_adam_chunk_bytes() bytes each, n <=
 * i3d_adam_chunk_elems()); steps: the n_steps per-parameter step counters (fp32), incremented by the launch;
 * bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t) for the step t being taken.
 * The update is torch's fused Adam expression for expression (L2 weight decay; no amsgrad / maximize / grad scaling). */
int i3d_adam_chunk_elems(void);
int i3d_adam_chunk_bytes(void);
int i3d_adam_step(const void* chunk_table, int n_chunks, float* steps, int n_steps, double lr, double beta1, double beta2,
                  double weight_decay, double eps, double bias_correction1, double bias_correction2_sqrt, void* stream);

/* ---- moving average of all teacher parameters of a BYOL wrapper in one launch, in place (csrc/ema.hip; reference
 * trainer/byol_wrapper.py:38-40).  chunk_table: device array of n_chunks records {float* teacher, const float* student, int n,
 * int pad} (i3d_ema_chunk_bytes() bytes each, n <= i3d_ema_chunk_elems()).  Per element, with three roundings as in the
 * reference's expression and no fused multiply-add:  teacher = fl(fl(teacher * decay) + fl(student * one_minus_decay));
 * the caller passes decay = (float)d and one_minus_decay = (float)(1.0 - d), the subtraction in double. */
int i3d_ema_chunk_elems(void);
int i3d_ema_chunk_bytes(void);
int i3d_ema_update(const void* chunk_table, int n_chunks, float decay, float one_minus_decay, void* stream);

/* ---- contrastive monitoring metrics -------------------------------------------------
 * replaces the nine metric modules of configs_clean/pre-train_QM9.yml:15-24 (reference trainer/metrics.py:161-174,
 * 212-333, 443-463; commons/losses.py:946-959), evaluated every log_iterations steps by
 * trainer/self_supervised_trainer.py:31-50.  One call per pair of tensors z1 [B1, D1], z2 [B2, D2]; every statistic from CENTRED
 * values (column means in fp64 first; pairwise distances from the Gram matrices of the centred rows; alignment and row norms from
 * the rows themselves; covariance from c^T c), the five products on i3d_gemm_f32_ex pinned to exact fp32 products and one K-slice
 * whatever i3d_set_matmul_precision / i3d_set_fp32_products say (both are restored before the call returns; as they are process-level,
 * a GEMM issued by ANOTHER host thread during the call would see the pinned values).  Fixed summation orders, no atomics.
 * pairwise != 0 (D1 == D2, B2 >= B1: the rows of z2 from B1 on are appended "noisy" samples): all statistics; pairwise == 0: the
 * per-tensor ones (out[0..7] = 0).  work: i3d_contrastive_metrics_work_floats floats (16-byte aligned).
 * out (fp64, i3d_contrastive_metrics_out_doubles(D1, D2) doubles):
 *   [0..7] sums over the rows i of {sum_j cos_ij, cos_ii, [(cos_ii+1)/2 > threshold], #{j != i: (cos_ij+1)/2 <= threshold},
 *          |z1_i - z2_i|^alpha, sum_{j>i} exp(-t|z1_i-z1_j|^2), the same for z2 (all B2 rows),
 *          <z1_i, z2_i> / (max(|z1_i|, 1e-8) max(|z2_i|, 1e-8)) (F.cosine_similarity)}, cos = <z1_i, z2_j> / (|z1_i| |z2_j|)
 *   [8], [9] per view sum_{a != b} (cov_ab)^2, cov = c^T c / (n - 1)
 *   then mean1 [D1] | var1 [D1] | mean2 [D2] | var2 [D2] (unbiased, from centred squares) | D1 + D2 doubles of scratch. */
long i3d_contrastive_metrics_out_doubles(int D1, int D2);
long i3d_contrastive_metrics_work_floats(int B1, int B2, int D1, int D2, int pairwise);
int i3d_contrastive_metrics(const float* z1, const float* z2, int B1, int B2, int D1, int D2, int pairwise, float threshold, float t,
                            float alpha, float* work, double* out, void* stream);

/* ---- batch assembly -----------------------------------------------------------------
 * replaces B x QM9Dataset.get_complete_graph (reference datasets/qm9_dataset.py:233-244, :215-217) + dgl.batch
 * (datasets/custom_collate.py:108-109) for the 3D view: from coords [N,3] and the node offsets graph_ptr[B+1] (plus
 * edge_ptr[B+1], the prefix sum of n(n-1)) builds, on the device, the complete graphs in the reference's edge-id
 * order (src_id/dst_id int64 [E3], d_id fp32 [E3] = ||x_src-x_dst||) AND the destination-sorted kernel index
 * (in_ptr[N+1] (== out_ptr), src_s, dst_s, perm, inv_perm, out_epos: int32 [E3]). */
int i3d_complete_graph_build(const float* coords, const int* graph_ptr, const int* edge_ptr, int num_graphs,
                             int num_nodes, int num_edges, int* in_ptr, int* src_s, int* dst_s, int* perm,
                             int* inv_perm, int* out_epos, int64_t* src_id, int64_t* dst_id, float* d_id,
                             void* stream);

/* ---- distance-prediction baseline (reference models/distance_predictor.py; csrc/distance.hip) ------------------------
 * i3d_mha_fwd: the self-attention of torch.nn.TransformerEncoderLayer(batch_first=True) over the atoms of each molecule, the
 *   molecules given as node ranges [graph_ptr[g], graph_ptr[g+1]) (g < num_graphs) instead of a padded batch with a key
 *   padding mask (reference distance_predictor.py:50-58).  qkv [N, 3 hidden]: q | k | v rows of the in_proj product (bias
 *   included), head h at columns h*dh .. h*dh+dh-1 of each third, dh = hidden / nhead <= 128.  out [N, hidden] =
 *   softmax(scale q k^T) v per (molecule, head), heads concatenated (the input of out_proj); lse [N, nhead] = the row's
 *   log-sum-exp of scale q k^T, kept for the backward pass.  scale = 1 / sqrt(dh) for torch's attention.
 * i3d_mha_bwd: grad_qkv [N, 3 hidden] (dQ | dK | dV; every element written) from grad_out [N, hidden] with P recomputed from
 *   qkv and lse; delta [N, nhead] is scratch (rowsum(grad_out * out) per head).
 * i3d_ln_res_fwd: y = LayerNorm(x + r) * gamma + beta over rows of `feat` columns (biased variance, eps added inside the
 *   square root), mean / rstd [rows] saved.
 * i3d_ln_res_bwd: grad_x [rows, feat] (the gradient of x and of r alike), grad_gamma / grad_beta [feat] as column sums through
 *   `partial` (i3d_ln_res_partial_floats(rows, feat) floats): per block of rows, then over the blocks in order.
 * Pair head over the ordered pairs of a pair graph (the complete graph of every molecule: the pairwise_indices of reference
 * datasets/custom_collate.py:65-78) in its destination-sorted order e: (i, j) = (src_s[e], dst_s[e]), pair id perm[e]:
 * i3d_pair_sum_fwd: out[perm[e], c] = softplus(u[i, c] + u[j, c] + 2 bias[c]), u [N, feat] (distance_net of one Linear, whose
 *   two calls on [h_i | h_j] and [h_j | h_i] add up to (W_a + W_b) h_i + (W_a + W_b) h_j + 2 b); out [pairs, feat].
 * i3d_pair_sum_bwd: grad_pair[e, c] = grad_out[perm[e], c] * sigmoid(u[i, c] + u[j, c] + 2 bias[c]), [pairs, feat], e order.
 * i3d_pair_norm_fwd: out[perm[e]] = ||p[i] - p[j]||_2, p [N, feat], out [pairs].
 * i3d_pair_norm_bwd: grad_pair [pairs, 2 feat], e order: columns 0..feat-1 the gradient w.r.t. p[i], columns feat..2 feat-1
 *   the one w.r.t. p[j]; 0 where the distance is 0.  The per-node sums of grad_pair are i3d_segment_sum over the pair graph's
 *   out_ptr / out_epos (source side) and in_ptr (destination side). */
int i3d_mha_fwd(const float* qkv, const int* graph_ptr, int num_graphs, int num_nodes, int hidden, int nhead, float scale,
                float* out, float* lse, void* stream);
int i3d_mha_bwd(const float* qkv, const float* out, const float* grad_out, const float* lse, const int* graph_ptr,
                int num_graphs, int num_nodes, int hidden, int nhead, float scale, float* delta, float* grad_qkv,
                void* stream);
int i3d_ln_res_fwd(const float* x, const float* r, const float* gamma, const float* beta, int rows, int feat, float eps,
                   float* y, float* mean, float* rstd, void* stream);
long i3d_ln_res_partial_floats(int rows, int feat);
int i3d_ln_res_bwd(const float* grad_y, const float* x, const float* r, const float* gamma, const float* mean,
                   const float* rstd, int rows, int feat, float* grad_x, float* partial, float* grad_gamma, float* grad_beta,
                   void* stream);
int i3d_pair_sum_fwd(const float* u, const float* bias, const int* src_s, const int* dst_s, const int* perm, int pairs,
                     int feat, float* out, void* stream);
int i3d_pair_sum_bwd(const float* grad_out, const float* u, const float* bias, const int* src_s, const int* dst_s,
                     const int* perm, int pairs, int feat, float* grad_pair, void* stream);
int i3d_pair_norm_fwd(const float* p, const int* src_s, const int* dst_s, const int* perm, int pairs, int feat, float* out,
                      void* stream);
int i3d_pair_norm_bwd(const float* grad_out, const float* p, const float* dist, const int* src_s, const int* dst_s,
                      const int* perm, int pairs, int feat, float* grad_pair, void* stream);

/* ---- node-dropped views (GraphCL baseline; csrc/nodedrop.hip) -------------------------------------------------------
 * replaces NodeDropCollate (reference datasets/custom_collate.py:230-263: per graph and view, remove_nodes(randperm(n)[:k]),
 * then dgl.batch) for a batch already on the device.  DGL's remove_nodes semantics: kept nodes renumbered in ascending order,
 * every edge touching a removed node dropped, kept edges in their relative order, node / edge features sliced to match.
 * Input: a block-diagonal batch in the layout of FlatMolDataset.assemble_host: src / dst int64 [E] (edge-id order),
 * atom_feat int64 [N, atom_cols], bond_feat int64 [E, bond_cols], and its kernel index (in_ptr, perm, src_s, dst_s, out_ptr,
 * out_epos, graph_ptr [num_graphs + 1]).  Per view, the host supplies the keep mask and what it counted from it: the view's
 * node / edge offsets per molecule, the first deg_rows slot of every (molecule g, in-degree D) at deg_base[g * deg_stride + D]
 * (D < deg_stride <= 64), and the -1 padding ranges of the degree groups.  Every output array of a view is written: src, dst,
 * atom_feat [N', atom_cols], bond_feat [E', bond_cols], the index (in_ptr / out_ptr [N' + 1], perm, src_s, dst_s, out_epos,
 * inv_perm [E']) and deg_rows [rows], identical to graph.build_index / group_nodes_by_degree(include_zero=True) of the dropped
 * batch; the view's graph_ptr is its input.  One wave per (molecule, view), one launch, no atomics.  max_atoms / max_edges:
 * bounds of the molecules' sizes (LDS: 4 (max_atoms + 3 max_edges + 2) bytes <= 64 KiB).  A molecule whose kept counts
 * differ from the view's offsets is not written. */
typedef struct {
    const unsigned char* keep;  /* [N] 1: node kept, 0: removed */
    const int* graph_ptr;       /* [num_graphs + 1] node offsets of the view */
    const int* edge_ptr;        /* [num_graphs + 1] edge offsets of the view */
    const int* deg_base;        /* [num_graphs, deg_stride] */
    const int* pad_range;       /* [n_groups, 2] [begin, end) of the -1 padding of each degree group */
    int n_groups, num_nodes, num_edges, rows;
    int64_t *src, *dst, *atom_feat, *bond_feat;
    int *in_ptr, *perm, *src_s, *dst_s, *out_ptr, *out_epos, *inv_perm, *deg_rows;
} I3dNodeDropView;
int i3d_node_drop_build(const int64_t* src, const int64_t* dst, const int64_t* atom_feat, const int64_t* bond_feat,
                        const int* in_ptr, const int* perm, const int* src_s, const int* dst_s, const int* out_ptr,
                        const int* out_epos, const int* graph_ptr, int num_graphs, int atom_cols, int bond_cols,
                        int max_atoms, int max_edges, int deg_stride, const I3dNodeDropView* views, int n_views,
                        void* stream);

/* ---- noised-3D negatives (csrc/noised3d.hip) ---------------------------------------------------------------------------
 * replaces NoisedDistancesCollate / NoisedCoordinatesCollate (reference datasets/custom_collate.py:131-152, :160-185: U deep
 * copies of the batched 3D graph, each noised, then dgl.batch of the 1 + U graphs) for the complete graphs of a batch: ONE
 * launch builds the whole (1 + U)-fold batch from the inputs of i3d_complete_graph_build.  Copy-major: molecule g of copy c is
 * graph c B + g, offset by c N nodes and c E3 edges; copy 0 is the clean batch, bitwise what i3d_complete_graph_build writes.
 * Outputs, T = 1 + num_noised: in_ptr [T N + 1] (== out_ptr), src_s / dst_s / perm / inv_perm / out_epos int32 [T E3],
 * graph_ptr_out [T B + 1], src_id / dst_id int64 [T E3], d_id fp32 [T E3] and, in coordinates mode, x_out fp32 [T N, 3] (may
 * be null otherwise).  Every element is written by exactly one thread; no atomics.
 * I3D_NOISED_DISTANCES:   d = fl(|x_u - x_v|) + std z(c, e), an independent normal per directed edge, no clamp.
 * I3D_NOISED_COORDINATES: d = |(x_u + std z(c, u)) - (x_v + std z(c, v))|, one 3-vector per (copy, node); x_out holds the
 *   noised positions.
 * z: Philox4x32-10, key = (seed low word, seed high word), counter = (element, copy, step low word, step high word), element =
 * the clean batch's edge id (distances) or node id (coordinates); u(w) = ((w >> 8) + 0.5) 2^-24 rounded to fp32 (in (0, 1]);
 * z0 = sqrt(-2 ln u(w0)) cos(2 pi u(w1)), z1 = the sine partner, z2 = sqrt(-2 ln u(w2)) cos(2 pi u(w3)); distances mode takes z0,
 * coordinates mode (z0, z1, z2).  The stream is this builder's own: equal to torch.randn in distribution, not in values.
 * A total T E3 or T N + 1 beyond int32 is refused (I3D_ERR_INVALID, "does not fit the int32 index arrays"). */
#define I3D_NOISED_DISTANCES 0
#define I3D_NOISED_COORDINATES 1
int i3d_noised_graph_build(const float* coords, const int* graph_ptr, const int* edge_ptr, int num_graphs, int num_nodes,
                           int num_edges, int num_noised, int mode, float std_, unsigned long long seed,
                           unsigned long long step, int* in_ptr, int* src_s, int* dst_s, int* perm, int* inv_perm,
                           int* out_epos, int* graph_ptr_out, int64_t* src_id, int64_t* dst_id, float* d_id, float* x_out,
                           void* stream);

/* ---- 3D autoencoder (reference models/net3d_VAE.py, commons/losses.py:165-204; csrc/pairmlp.hip) -------------------
 * The pair head distance_net = FCLayer(2H -> D, ReLU, BatchNorm) -> FCLayer(D -> 1) of reference net3d_VAE.py:116-119
 * (projection_layers=2): softplus(f([h_s | h_d]) + f([h_d | h_s])) per ordered pair, each of the two calls with its own batch
 * statistics.  AB [N, 2 D] = h [W1a | W1b]^T is the node-level half of the first Linear (W1 = [W1a | W1b], one GEMM); the pairs
 * are the edges of a pair graph in its destination-sorted order e, (s, d) = (src_s[e], dst_s[e]), pair id perm[e] (any pair
 * list, symmetric or not).  x1 = relu(A[s] + B[d] + b1), x2 = relu(A[d] + B[s] + b1) are recomputed wherever they are needed:
 * no [P, 2H] or [P, D] tensor exists in either direction.  D = width <= 128 (i3d_pair_mlp_supported).
 * i3d_pair_mlp_fwd: out[perm[e]] = softplus(sum_c w2 BN_1(x1)[c] + w2 BN_2(x2)[c] + 2 b2), out [pairs].  training != 0: batch
 *   statistics (biased variance) from a blocked fp64 reduction through `workspace` (i3d_pair_mlp_workspace_floats(pairs,
 *   width) floats), running_mean / running_var updated with the s->d statistics first and the d->s statistics second (unbiased
 *   variance, `momentum`), num_batches_tracked (int64 on the device, may be null) + 2; pairs >= 2.  training == 0: the running
 *   estimates for both orders, no reduction, workspace unused.  stats [4, D] (mean1 | rstd1 | mean2 | rstd2) and coef [2 D + 1], fp64
 *   (constants shared by every pair of a column: their rounding would shift all pairs alike),
 *   are outputs, and inputs of the backward pass.  pairs == 0: nothing is launched.
 * i3d_pair_mlp_bwd: from grad_out [pairs] and the forward's stats and coef (o_e, the argument of the softplus, is recomputed
 *   as the forward computed it): grad_gamma, grad_beta, grad_w2
 *   [D], grad_b2 [1] and grad_AB [num_nodes, 2 D] (every row written; dh, dW1 and db1 follow on the GEMMs: dh = dA W1a + dB W1b,
 *   dW1 = [dA^T h | dB^T h], db1 = colsum(dA)).  grad_pair [pairs] (do_e, e order) and bcoef [6 D + 1] (fp64) are scratch; workspace as
 *   in the forward.  Per node, the in-pairs are summed first (in_ptr), then the out-pairs (out_ptr / out_epos); all sums have
 *   a fixed order, no atomics.  `training` as in the forward.  pairs >= 1.
 * i3d_mse_fwd: loss[0] = scale * sum_i (a[i] - b[i])^2 (scale = weight / n for torch.nn.MSELoss times the reference's
 *   reconstruction_reg, commons/losses.py:204) through `partial` (i3d_mse_partial_floats(n) floats): differences, squares and
 *   sums in fp64, blocks summed in order, rounded once.
 * i3d_mse_bwd: grad_a[i] = 2 scale g (a[i] - b[i]), grad_b = -grad_a (either may be null), g = grad_scale[0] read on the
 *   device (null: 1). */
int i3d_pair_mlp_supported(int width);
long i3d_pair_mlp_workspace_floats(int pairs, int width);
int i3d_pair_mlp_fwd(const float* AB, const float* b1, const float* gamma, const float* beta, const float* w2, const float* b2,
                     const int* src_s, const int* dst_s, const int* perm, int pairs, int width, int training, float eps,
                     float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, double* stats,
                     double* coef, float* workspace, float* out, void* stream);
int i3d_pair_mlp_bwd(const float* grad_out, const double* coef, const float* AB, const float* b1, const float* gamma,
                     const float* beta, const float* w2, const int* src_s, const int* dst_s, const int* perm, const int* in_ptr,
                     const int* out_ptr, const int* out_epos, int num_nodes, int pairs, int width, int training,
                     const double* stats, float* workspace, float* grad_pair, double* bcoef, float* grad_AB, float* grad_gamma,
                     float* grad_beta, float* grad_w2, float* grad_b2, void* stream);
long i3d_mse_partial_floats(long n);
int i3d_mse_fwd(const float* a, const float* b, long n, double scale, float* partial, float* loss, void* stream);
int i3d_mse_bwd(const float* a, const float* b, long n, double scale, const float* grad_scale, float* grad_a, float* grad_b,
                void* stream);

/* ---- multi-conformer losses with one 2D embedding per conformer (reference commons/losses.py:394-476, 692-744; csrc/sep2d.hip) ----
 * B = batch molecules, C = conf conformers (1..i3d_sep2d_max_conformers() = 8), N = B C points per view, D = dim features.  Both
 * views are [N, D], molecule major.  Every sum has a fixed order, no atomics; nothing of size B^2 C^2 D exists.
 * i3d_row_normalize_fwd: y = x / max(|x|, 1e-12) per row (torch F.normalize), norms[r] = |x_r| (before the clamp).
 * i3d_row_normalize_bwd: grad_x = (grad_y - y (y . grad_y)) / |x|; rows below the clamp: grad_y / 1e-12.
 * i3d_sep2d_fwd: sim [N, N] = z1v z2^T (rows (i, l), columns (j, u)), n1 / n2 [N] the row norms (ones: no normalisation), no
 *   epsilon.  P = exp(sim / (n1 n2) / tau); row_den[i] = sum of P over the rows of molecule i and the columns of every OTHER
 *   molecule, row_pos[i] = sum_l P[(i, l), (i, l)] (fp64, [B]); loss[0] = -mean_i log(row_pos / row_den).
 * i3d_sep2d_bwd: dsim = dL/d sim [N, N] and the norm-path coefficients ca, cb [N] (dz1 = dsim z2 + ca z1v, dz2 = dsim^T z1v +
 *   cb z2), times grad_scale[0] read on the device (null: 1).
 * i3d_mmd_pair_fwd: X = the 2D view, Y = the 3D view (normalised by the caller).  Entry [a, b] of sim / bandwidth [B, B] compares
 *   the 2C points X[b] followed by Y[a]: cross [N, N] with cross[(a, u), (b, l)] = |Y[a, u] - X[b, l]|^2 and intra [2, B, C, C]
 *   (0: X, 1: Y) by direct differences; bandwidth = (sum of all (2C)^2 squared distances) / ((2C)^2 - 2C) / kernel_mul^(kernel_num / 2);
 *   K(L) = sum_{k < kernel_num} exp(-L / (bandwidth kernel_mul^k)); mmd = mean over C x C of K_XX + K_YY - K_XY - K_YX;
 *   sim = 1 / (mmd + 1).  cross, intra, bandwidth and sim are outputs, and inputs of the backward pass.
 * i3d_mmd_pair_bwd: from dsim [B, B], with the bandwidth held constant: dX, dY [N, D].  gcross [N, N] and gintra [2, B, C, C] are
 *   scratch. */
int i3d_row_normalize_fwd(const float* x, int rows, int dim, float* y, float* norms, void* stream);
int i3d_row_normalize_bwd(const float* x, const float* norms, const float* grad_y, int rows, int dim, float* grad_x, void* stream);
int i3d_sep2d_max_conformers(void);
int i3d_sep2d_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, float tau, double* row_den,
                  double* row_pos, float* loss, void* stream);
int i3d_sep2d_bwd(const float* sim, const float* n1, const float* n2, const double* row_den, const double* row_pos, int batch,
                  int conf, float tau, const float* grad_scale, float* dsim, float* ca, float* cb, void* stream);
int i3d_mmd_pair_fwd(const float* X, const float* Y, int batch, int conf, int dim, int kernel_num, double kernel_mul, float* cross,
                     float* intra, float* bandwidth, float* sim, void* stream);
int i3d_mmd_pair_bwd(const float* X, const float* Y, const float* cross, const float* intra, const float* bandwidth,
                     const float* sim, const float* dsim, int batch, int conf, int dim, int kernel_num, double kernel_mul,
                     float* gcross, float* gintra, float* dX, float* dY, void* stream);

/* ---- KLDivergenceMultiplePositives (reference commons/losses.py:261-314; csrc/klmp.hip) ----
 * z1 [B, 2 D]: per molecule the mean m1 (columns 0..D-1) and the log-variance s1 (columns D..2D-1) of a diagonal Gaussian; z2 [B C, D],
 * molecule major: m2 = mean over the C conformers, v2 = their unbiased variance (two-pass) + 1e-6.  B = batch >= 1, C = conf >= 2
 * (no upper limit), D = dim >= 1; anything else returns I3D_ERR_INVALID before a launch.
 * i3d_kl_mp_fwd: stats [B, 3] (fp64) = per molecule { kl_b = 0.5 sum_d (s1 - log v2 + (v2 + (m2 - m1)^2) exp(-s1) - 1),
 *   sum_d var(z2_b) (without the 1e-6), sum_d exp(s1_b) }; loss[0] = inv_global_batch sum_b kl_b in a fixed order (loss null: the
 *   statistics only).
 * i3d_kl_mp_bwd: recomputes m2 and v2 and writes every entry of dz1 [B, 2 D] and dz2 [B C, D], times inv_global_batch and
 *   grad_scale[0] read on the device (null: 1).  No atomics, no scratch. */
int i3d_kl_mp_fwd(const float* z1, const float* z2, int batch, int conf, int dim, double inv_global_batch, double* stats, float* loss,
                  void* stream);
int i3d_kl_mp_bwd(const float* z1, const float* z2, int batch, int conf, int dim, double inv_global_batch, const float* grad_scale,
                  float* dz1, float* dz2, void* stream);

/* ---- NTXentLikelihoodLoss, PositiveProb / NegativeProb, JSDMultiplePositivesLoss (reference commons/losses.py:537-595, :317-391,
 * trainer/metrics.py:336-395; csrc/gausspair.hip) ----
 * z1 [B, 2 D] as above (mean m | log-variance s); B = batch >= 2, D = dim >= 1, C = conf >= 1 (likelihood) or >= 2 (JSD), no upper
 * limit on C and D; anything else returns I3D_ERR_INVALID before a launch.  Every term in fp64, fixed summation order, no atomics, no
 * buffer beyond [B, B] doubles.
 * i3d_gauss_lik_fwd: lik [B, B] (fp64), lik[i, j] = 1 / (C D) sum_{c, d} N(x; m_id, exp(s_id)) with x = z2[j mol_stride + c conf_stride
 *   + d]: the mean over conformers and features of the per-dimension densities.  z2 holds B C D floats; the strides (in floats) are
 *   those of the molecule-major layout (C D, D) or of the conformer-major one (D, B D), nothing else.
 * i3d_gauss_lik_loss: rows [B, 2] (fp64) = per row { log den_i = log sum_{j != i} exp(lik_ij / tau), l_i = log den_i - lik_ii / tau }
 *   - the negatives are summed directly and the row maximum leaves the exponent -, loss[0] = mean_i l_i.
 * i3d_gauss_lik_probs: out (2 doubles) = { mean_i lik_ii, mean_i sum_{j != i} lik_ij }.
 * i3d_gauss_lik_bwd: grad_lik [B, B] (fp64, scratch) = d loss / d lik times grad_scale[0] read on the device (null: 1); dz1 [B, 2 D] and
 *   dz2 (the layout of z2) from one owner thread per output element, both passes recompute the densities.
 * i3d_gauss_jsd_fwd: z2 molecule major; m2 / v2 = mean / unbiased variance over the conformers (two-pass, no epsilon).  astat [B, 2] =
 *   per molecule { product over d of the non-zero v2, number of zero v2 }; sim [B, B], rows a: 3D view, columns b: 2D view,
 *   sim[a, b] = 0.5 (log(prod_d v2_ad + 1e-5) - sum_d s_bd - D + sum_d (exp(s_bd) + (m2_ad - m1_bd)^2) / (v2_ad + 1e-5));
 *   rows [B, 3] = { sim_aa, den_a = sum_{b != a} sim_ab, -log(sim_aa / den_a) }; loss[0] = the mean of the last (NaN where the ratio is
 *   negative).
 * i3d_gauss_jsd_bwd: dz1 [B, 2 D] and dz2 [B C, D] from astat and rows, times grad_scale[0] read on the device (null: 1). */
int i3d_gauss_lik_fwd(const float* z1, const float* z2, int batch, int conf, int dim, long mol_stride, long conf_stride, double* lik,
                      void* stream);
int i3d_gauss_lik_loss(const double* lik, int batch, double tau, double* rows, float* loss, void* stream);
int i3d_gauss_lik_probs(const double* lik, int batch, double* out, void* stream);
int i3d_gauss_lik_bwd(const float* z1, const float* z2, int batch, int conf, int dim, long mol_stride, long conf_stride,
                      const double* lik, const double* rows, double tau, const float* grad_scale, double* grad_lik, float* dz1,
                      float* dz2, void* stream);
int i3d_gauss_jsd_fwd(const float* z1, const float* z2, int batch, int conf, int dim, double* astat, double* sim, double* rows,
                      float* loss, void* stream);
int i3d_gauss_jsd_bwd(const float* z1, const float* z2, int batch, int conf, int dim, const double* astat, const double* rows,
                      const float* grad_scale, float* dz1, float* dz2, void* stream);

/* ---- fine-tuning: NaN-label losses and one-pass task moments (csrc/task.hip) ----
 * pred, target [rows, tasks] row major (fp32), rows >= 1, tasks >= 1; anything else returns I3D_ERR_INVALID before a launch.
 * i3d_masked_loss_fwd: stands for `self.bce_loss(pred[is_labeled], target[is_labeled])` / `self.mse_loss(...)` of reference
 *   commons/losses.py:17-21, 27-31 (OGBNanLabelBCEWithLogitsLoss, OGBNanLabelMSELoss).  kind 0: BCE with logits in torch's stable form
 *   max(x, 0) - x t + log1p(exp(-|x|)); kind 1: (x - t)^2.  An element is labelled iff its target is not NaN; pred at an unlabelled
 *   position never reaches the result.  out (3 doubles): out[0] = the mean over the labelled elements (NaN when there is none),
 *   out[1] = their count, the first four bytes of out[2] = out[0] rounded to fp32 (the loss tensor).  partials:
 *   i3d_masked_loss_partial_floats(rows, tasks) floats, 8-byte aligned.  Terms and sums in fp64, fixed order, no atomics.
 * i3d_masked_loss_bwd: the backward of the same call sites (the reference's index-put): grad_pred = grad_out[0] (sigmoid(x) - t) /
 *   count (kind 0) or grad_out[0] 2 (x - t) / count (kind 1) where labelled, exactly 0.0f elsewhere; count = out[1] of the forward
 *   and grad_out (null: 1) are read on the device.
 * i3d_task_moments: stands for the per-metric reductions of reference trainer/metrics.py:23-32 (PearsonR), :48-54, :66-70, :98-101
 *   (QM9SingleTargetDenormalizedL1, QM9DenormalizedL1, QM9DenormalizedL2), :77-79 (MAE), :142-145 (Rsquared) and :157-158
 *   (MeanPredictorLoss), which Trainer.evaluate_metrics (trainer/trainer.py:174-183) runs one after the other.  table [tasks + 1][10]
 *   (fp64), per task c: { n, sum p, sum t, sum (p - pbar_c)^2, sum (t - tbar_c)^2, sum (p - pbar_c)(t - tbar_c), sum |p - t|,
 *   sum (p - t)^2, sum |t - tbar|, sum (t - tbar)^2 }, pbar_c / tbar_c the column means, tbar the mean of all targets; row `tasks`
 *   holds the column totals.  Two passes (means first), four launches, no masking: NaN propagates as in the reference.  partials:
 *   i3d_task_moments_partial_floats(rows, tasks) floats, 8-byte aligned. */
long i3d_masked_loss_partial_floats(int rows, int tasks);
int i3d_masked_loss_fwd(const float* pred, const float* target, int rows, int tasks, int kind, float* partials, double* out,
                        void* stream);
int i3d_masked_loss_bwd(const float* pred, const float* target, int rows, int tasks, int kind, const double* out,
                        const float* grad_out, float* grad_pred, void* stream);
long i3d_task_moments_partial_floats(int rows, int tasks);
int i3d_task_moments(const float* pred, const float* target, int rows, int tasks, float* partials, double* table, void* stream);

/* ---- GIN message step of the OGBGNN baseline (reference models/gin.py; csrc/gin.hip) ----
 * N = num_nodes >= 1, E = num_edges >= 0, H = feat >= 1, V = num_codes in 1..256; anything else returns I3D_ERR_INVALID before a
 * launch.  Edge arrays are in destination-sorted order (graph.GraphIndex); T [V, H] is the table of the bond embeddings of all V
 * feature combinations and codes [E] names every edge's row (i3d_edge_codes); eps is a device scalar.  Rows are read four floats
 * at a time when H % 4 == 0 and the buffers are 16-byte aligned, else one at a time.  Fixed summation order, no atomics, no [E, H]
 * buffer in either direction.
 * i3d_gin_conv_fwd: stands for `h_list[layer] + virtualnode_embedding[batch_id]` (models/gin.py:276) and GINConv.forward up to the
 *   MLP (models/gin.py:103-108: bond_encoder, copy_u, relu(m + edge_embedding), sum, (1 + eps) x + new_x).  vn [B, H] with
 *   graph_ptr [B + 1]: x = h + vn[graph of the node] is written to x [N, H]; vn null: x is h and the x argument is not touched.
 *   z[v] = (1 + eps) x[v] + sum over the in-edges e of v (in_ptr order) of relu(x[src(e)] + T[codes[e]]).  The source of an edge
 *   lies in the molecule of its destination.  One launch.
 * i3d_gin_conv_bwd: the backward of the same lines from g = dL/dz [N, H], x as the forward left it (h without a virtual node):
 *   dx[u] = (1 + eps) g[u] + sum over the out-edges e of u (out_ptr / out_epos order) of g[dst(e)] [x[u] + T[codes[e]] > 0];
 *   dT[c] = sum over the edges of code c of g[dst(e)] [x[src(e)] + T[c] > 0], a zero row for a code without edges;
 *   deps[0] = sum_v <g[v], x[v]>.  dT and deps are summed in fp64 and rounded once.  code_order [E]: the edge positions sorted by
 *   code (stable), code_ptr [V + 1]: where every code's run starts in it; dT is reduced over chunks of i3d_gin_chunk_edges()
 *   positions of that list, then per code in chunk order.  partials: i3d_gin_conv_bwd_partial_floats(N, E, H, V) floats, 8-byte
 *   aligned.  Three launches (two when E = 0). */
int i3d_gin_chunk_edges(void);
long i3d_gin_conv_bwd_partial_floats(int num_nodes, int num_edges, int feat, int num_codes);
int i3d_gin_conv_fwd(const float* h, const float* vn, const int* graph_ptr, int num_graphs, const float* T, int num_codes,
                     const int* codes, const int* in_ptr, const int* src_s, const float* eps, int num_nodes, int num_edges, int feat,
                     float* x, float* z, void* stream);
int i3d_gin_conv_bwd(const float* g, const float* x, const float* T, int num_codes, const int* codes, const int* src_s,
                     const int* dst_s, const int* out_ptr, const int* out_epos, const int* code_order, const int* code_ptr,
                     const float* eps, int num_nodes, int num_edges, int feat, float* partials, float* dx, float* dT, float* deps,
                     void* stream);

/* ---- EGNN: soft-edge gate, in-edge reduction and residual add in one launch per direction (reference models/egnn.py:124-137;
 * csrc/egnn.hip) ----
 * N = num_nodes >= 1, E = num_edges >= 0, H = feat >= 1; anything else returns I3D_ERR_INVALID before a launch.  m [E, H] is in
 * destination-sorted order, ws [H] and bs [1] are soft_edge_network's weight and bias, in_ptr [N + 1].  The kernels cover
 * H % 4 == 0, H <= i3d_gate_reduce_max_feat() (512) and 16-byte aligned m, ws, h, u, gu, gm, part_ws; every other valid call
 * returns I3D_NOT_TAKEN and the caller composes the step from i3d_soft_edge_*, i3d_segment_sum / i3d_segment_bcast and i3d_add.
 * One wave per destination, fixed summation order, no atomics, no [E, H] buffer besides m and its gradient.
 * i3d_gate_reduce_fwd: w[j] = sigmoid(<ws, m[j]> + bs) [E];  u[v] = h[v] + sum over the in-edges j of v of m[j] w[j], the sum
 *   divided by the in-degree when reduce_mean != 0 (DGL fn.mean); a node without in-edges gets u[v] = h[v].  One launch.
 * i3d_gate_reduce_bwd: from gu = dL/du [N, H], m and the w of the forward: g = gu[dst(j)] (over the in-degree for the mean),
 *   gg_j = <g, m[j]> w_j (1 - w_j), gm[j] = g w_j + gg_j ws [E, H];  part_ws [N, H] row v = sum over the in-edges of v of
 *   gg_j m[j], part_bs [N] entry v = the sum of gg_j (zeros without in-edges): their column sums over the nodes (i3d_colsum) are
 *   dL/dws and dL/dbs.  dL/dh = gu.  One launch. */
int i3d_gate_reduce_max_feat(void);
int i3d_gate_reduce_fwd(const float* m, const float* ws, const float* bs, const int* in_ptr, const float* h, int num_nodes,
                        int num_edges, int feat, int reduce_mean, float* u, float* w, void* stream);
int i3d_gate_reduce_bwd(const float* gu, const float* m, const float* w, const float* ws, const int* in_ptr, int num_nodes,
                        int num_edges, int feat, int reduce_mean, float* gm, float* part_ws, float* part_bs, void* stream);

/* ---- GeoMol's message-passing step (reference models/geomol_mpnn.py:72-74, :93-99; csrc/geomol.hip) ----
 * N = num_nodes >= 1, E = num_edges >= 0, H = feat >= 1, rows >= 0; anything else returns I3D_ERR_INVALID before a launch.  Edge
 * arrays and edge rows are in destination-sorted order (graph.GraphIndex).  fp32; rows are read four floats at a time when the width
 * allows and the buffers are 16-byte aligned, else one at a time: any H is taken.  Fixed summation order, no atomics, no buffer
 * beyond the caller's.
 * i3d_geomol_edge_fwd: h[j] = relu((F[j] + P[src_s[j]]) + Q[dst_s[j]]), F [E, H] (the bias of the edge Linear already in it),
 *   PQ [N, 2H]: row v = P[v] | Q[v], the product x [W_node_in | W_node_out]^T.  One launch (none when E = 0).
 * i3d_geomol_edge_bwd: from g = dL/dh [E, H] and the h of the forward (gate h > 0, strict):  dF[j] = g[j] gate [E, H], written
 *   once;  dPQ [N, 2H]: row v = dP[v] | dQ[v], dP[v] the sum of dF over the out-edges of v in out_ptr / out_epos order, dQ[v] the sum
 *   over its in-edges in in_ptr order; a zero half-row for a node without such edges.  ONE launch, E = 0 included.
 * i3d_geomol_residual_fwd: out = (1 + eps[0]) a + b on [rows, H]; eps is a device scalar (edge_eps / node_eps), 1 + eps an fp32
 *   sum.  One launch (none when rows = 0).
 * i3d_geomol_residual_bwd: da = (1 + eps[0]) g;  deps[0] = <g, a> accumulated in fp64 per workgroup, the workgroups' partials
 *   summed in workgroup order and rounded once.  dL/db is g itself.  partials: I3D_GEOMOL_PARTIAL_FLOATS floats, 8-byte aligned.
 *   Two launches (one when rows = 0: deps = 0). */
#define I3D_GEOMOL_PARTIAL_FLOATS 2048
int i3d_geomol_edge_fwd(const float* F, const float* PQ, const int* src_s, const int* dst_s, int num_nodes, int num_edges, int feat,
                        float* h, void* stream);
int i3d_geomol_edge_bwd(const float* g, const float* h, const int* in_ptr, const int* out_ptr, const int* out_epos, int num_nodes,
                        int num_edges, int feat, float* dF, float* dPQ, void* stream);
int i3d_geomol_residual_fwd(const float* a, const float* b, const float* eps, long rows, int feat, float* out, void* stream);
int i3d_geomol_residual_bwd(const float* g, const float* a, const float* eps, long rows, int feat, float* partials, float* da,
                            float* deps, void* stream);

/* ---- local-global NT-Xent: every node embedding against the graph embeddings (reference commons/losses.py:1117-1185;
 * csrc/localglobal.hip) ----
 * zn [n, dim] node embeddings, zg [b, dim] graph embeddings, graph_ptr [b + 1] int32: the nodes of graph j are the rows
 * graph_ptr[j] .. graph_ptr[j + 1] - 1 (a graph may be empty).  g(i) = the segment that holds row i (upper bound - 1, clamped to
 * [0, b - 1]: no content of graph_ptr makes a kernel read or write out of bounds).
 *   s'_ij = zn_i . zg_j / (|zn_i| |zg_j| + eps)   (norm == 0: the plain dot product, eps unused)
 *   loss  = mean_i ( log sum_{j != g(i)} exp(s'_ij / tau)  -  s'_{i g(i)} / tau )
 * The negatives are summed over the columns other than g(i) with their maximum taken out: finite wherever fp32 holds the result.
 * n >= 1, b >= 2, dim >= 1, tau > 0 and non-null pointers, anything else returns I3D_ERR_INVALID before a launch.
 * Deterministic: fixed summation orders that depend on (n, b, dim) only, no atomics.
 * i3d_lg_ntxent_scratch_floats: floats of `scratch`, written by _fwd and read by _bwd (row norms, per-row log-sum, row losses,
 *   the [n, b] similarity).  i3d_lg_ntxent_work_floats: floats of `work` of _bwd (dL/dsim [n, b], the per-chunk column partials
 *   [ceil(n / i3d_lg_row_chunk()), b] and the slices of the K = n product).
 * i3d_lg_ntxent_fwd: row norms, zn zg^T (i3d_gemm_f32), the row kernel, the sum of the n row losses in fp64 -> loss [1].
 * i3d_lg_ntxent_bwd: dzn [n, dim], dzg [b, dim] of grad_scale_dev[0] * loss (grad_scale_dev: one device float, or null = 1):
 *   dS'_ij = gs / (n tau) (j == g(i) ? -1 : e_ij / neg_i),  H = dS' / (a_i b_j + eps),  dzn = H zg + ca . zn,
 *   dzg = H^T zn + cb . zg with ca_i = -(1 / a_i) sum_j H_ij s'_ij b_j, cb_j = -(1 / b_j) sum_i H_ij s'_ij a_i; a zero row
 *   (a_i = 0 or b_j = 0) gets a zero norm term.  cb is reduced in two stages over row chunks of i3d_lg_row_chunk() rows. */
int i3d_lg_row_chunk(void);
long i3d_lg_ntxent_scratch_floats(int n, int b);
long i3d_lg_ntxent_work_floats(int n, int b, int dim);
int i3d_lg_ntxent_fwd(const float* zn, const float* zg, const int* graph_ptr, int n, int b, int dim, float tau, float eps,
                      int norm, float* scratch, float* loss, void* stream);
int i3d_lg_ntxent_bwd(const float* zn, const float* zg, const int* graph_ptr, int n, int b, int dim, float tau, float eps,
                      int norm, const float* scratch, const float* grad_scale_dev, float* work, float* dzn, float* dzg,
                      void* stream);

/* ---- set-matching and per-conformer NT-Xent (reference commons/losses.py:598-689, 747-794, 839-886; csrc/confmatch.hip) ----
 * B = batch >= 2 molecules, C = conf conformers, D = dim >= 1, tau > 0, s' = sim / (n1 n2) (n1, n2: the row norms, ones without
 * normalisation), no epsilon.  Anything else returns I3D_ERR_INVALID before a launch.  Fixed summation orders, no atomics.
 * Matching losses (C in 1..i3d_conf_match_max_conformers() = 8, N = B C <= 46340): sim [N, N] = z1v z2^T, rows (i, l), columns (j, u).
 *   mode 0, NTXentMinimumMatching: den_i = sum_{j != i} exp(min_{l, u} s'[(i, l), (j, u)] / tau), pos_i = exp(max over EVERY j and l
 *   of s'[(i, l), (j, l)] / tau) - the reference's amax over the matched diagonal runs over all column molecules.  mode 1,
 *   NTXentMaximumSimilarity: den_i = sum_{j != i} exp(max_{l, u} s' / tau), pos_i = exp(max_{l, u} s'[(i, l), (i, u)] / tau).
 *   loss[0] = -mean_i log(pos_i / den_i).  Ties: the lowest l, then the lowest u wins inside a molecule pair, the lowest j, then the
 *   lowest l among the candidates of the positive (torch splits a tie's gradient evenly; a tie has measure zero).  A NaN wins every
 *   selection.
 * i3d_conf_match_fwd: sel [B, B] bytes = l C + u of the selected entry of every molecule pair; dsel [B, B] bytes (mode 0 only, may
 *   be null in mode 1) = the l of the pair's largest matched entry; row_den, row_pos [B] (fp64); pos_j, pos_lu [B] (int32) = the
 *   column molecule and l C + u of the positive's entry.
 * i3d_conf_match_bwd: dz1 [N, D] (the gradient of z1v) and dz2 [N, D], times grad_scale[0] read on the device (null: 1), from one
 *   selected entry per molecule pair and one positive per molecule: no [N, N] gradient, no matrix product.  norm == 0: the norm
 *   terms are left out (n1 = n2 = ones).  work: i3d_conf_match_work_floats(B) floats.
 * Per-conformer losses (C in 1..i3d_per_conf_max_conformers() = 64, B^2 C < 2^31): sim [B, N] = z1 z2^T, z2 molecule major.
 *   mode 0, NTXentMultiplePositivesV2: pos_i = sum_u P[i, (i, u)], den_i = sum_{j != i} P[i, (j, 0)], den / pos [B].  mode 1,
 *   NTXentMultiplePositivesV3: pos_iu = P[i, (i, u)], den_iu = sum_{j != i} P[i, (j, u)], den / pos [B C].  P = exp(s' / tau);
 *   loss[0] = -mean log(pos / den) over the B (B C) terms.  The positives are left out of the sums, never subtracted.
 * i3d_per_conf_bwd: dsim = dL/d sim [B, N] (exact zeros where an entry is in no sum) and the norm-path coefficients ca [B], cb [N]
 *   (dz1 = dsim z2 + ca z1, dz2 = dsim^T z1 + cb z2), times grad_scale[0] read on the device (null: 1). */
int i3d_conf_match_max_conformers(void);
int i3d_per_conf_max_conformers(void);
long i3d_conf_match_work_floats(int batch);
int i3d_conf_match_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, int mode, float tau,
                       unsigned char* sel, unsigned char* dsel, double* row_den, double* row_pos, int* pos_j, int* pos_lu,
                       float* loss, void* stream);
int i3d_conf_match_bwd(const float* sim, const float* z1v, const float* z2, const float* n1, const float* n2,
                       const unsigned char* sel, const double* row_den, const int* pos_j, const int* pos_lu, int batch, int conf,
                       int dim, int mode, int norm, float tau, const float* grad_scale, float* work, float* dz1, float* dz2,
                       void* stream);
int i3d_per_conf_fwd(const float* sim, const float* n1, const float* n2, int batch, int conf, int mode, float tau, double* den,
                     double* pos, float* loss, void* stream);
int i3d_per_conf_bwd(const float* sim, const float* n1, const float* n2, const double* den, const double* pos, int batch, int conf,
                     int mode, float tau, const float* grad_scale, float* dsim, float* ca, float* cb, void* stream);

/* ---- single-positive losses with re-weighted negatives (csrc/hardneg.hip; reference commons/losses.py InfoNCE :998-1034, InfoNCEHard
 * :1037-1074, NTXentHard :1077-1114, NTXentExtraNegatives :889-943) ----
 * mode 0 InfoNCE, 1 NTXentHard, 2 InfoNCEHard, 3 NTXentExtraNegatives.  z1 [b1, dim] the local rows, z2 [b2, dim] the (gathered) other
 * view, the positive of row i is column pos_offset + i; x [b1 n_extra, dim] the private extra negatives of mode 3, row (i, u) at
 * i n_extra + u, n_extra in 0..i3d_hardneg_max_extra() = 256 (the other modes: 0, x null).  s' = <z1_i, z2_j> / (|z1_i||z2_j|) with no
 * epsilon (norm == 0: the plain product), P = exp(s' / tau), n = b2 - 1:
 *   pos_i = P[i, p_i], S_i = sum_{j != p_i} P_ij, A_i = sum_{j != p_i} P_ij^beta, C_i = sum_{j != p_i} P_ij^(1 + beta)
 *   mode 0: l_i = log(S_i + pos_i) - log pos_i
 *   mode 1: Ng_i = (n C_i / A_i - tau_plus n pos_i) / (1 - tau_plus), Ngc_i = max(Ng_i, n e^(-1 / tau)), l_i = log Ngc_i - log pos_i
 *   mode 2: l_i = log(pos_i + Ngc_i) - log pos_i
 *   mode 3: l_i = log(S_i + extra_weight sum_u Q_iu) - log pos_i, Q_iu = exp(<z1_i, x_iu> / (|z1_i||x_iu|) / tau)
 * loss[0] = loss_scale sum_i l_i.  The gradient runs through the importance weights P^beta.  mode in 0..3, b1, b2, dim >= 1, tau > 0,
 * pos_offset + b1 <= b2, modes 1 and 2: b2 >= 2 and tau_plus < 1; anything else returns I3D_ERR_INVALID before a launch.  Rows are read
 * four floats at a time when their length and the buffers' alignment allow, else one at a time.  Row sums in fp64 in a fixed order, no
 * atomics.
 * i3d_hardneg_norms: n1 [b1], n2 [b2] (ones when norm == 0) and, one wave per (i, u), xdot [b1 n_extra] = <z1_i, x_iu>, xn = |x_iu|.
 * i3d_hardneg_fwd: from sim [b1, b2] = z1 z2^T: stats [b1, 5] (fp64: pos, S, A, C - mode 3: sum_u Q_iu in C's place -, l), coef
 *   [b1, 4] (cp, c1, c2, cq: dl_i/dP P = cp at the positive, c1 P P^beta + c2 P^beta at a negative, cq Q at an extra negative) and loss.
 * i3d_hardneg_bwd: one launch: dsim = dL/d sim [b1, b2], the norm-path coefficients ca [b1], cb [b2] (null: not written) and - dz1,
 *   dz2 non-null - dz1 = ca z1 + the extra negatives' part, dz2 = cb z2, dx [b1 n_extra, dim]; all times grad_scale and
 *   grad_scale_dev[0] (null: 1).  dz1 += dsim z2 and dz2 += dsim^T z1 complete the gradients.
 * i3d_hardneg_loss_fwd / _bwd: the whole loss from one call per direction (norms, similarity GEMM, the row pass, the sum; the backward
 *   launch and the two GEMMs).  scratch: i3d_hardneg_loss_scratch_floats floats, 16-byte aligned, written by _fwd and read by _bwd;
 *   work: b1 * b2 floats, 16-byte aligned. */
int i3d_hardneg_max_extra(void);
int i3d_hardneg_norms(const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim, int norm, float* n1,
                      float* n2, float* xdot, float* xn, void* stream);
int i3d_hardneg_fwd(int mode, const float* sim, const float* n1, const float* n2, const float* xdot, const float* xn, int b1, int b2,
                    int n_extra, int pos_offset, double tau, double tau_plus, double beta, double extra_weight, double loss_scale,
                    double* stats, float* coef, float* loss, void* stream);
int i3d_hardneg_bwd(int mode, const float* sim, const float* n1, const float* n2, const float* coef, const float* xdot, const float* xn,
                    const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim, int pos_offset, int norm,
                    double tau, double beta, double grad_scale, const float* grad_scale_dev, float* dsim, float* ca, float* cb,
                    float* dz1, float* dz2, float* dx, void* stream);
long i3d_hardneg_loss_scratch_floats(int b1, int b2, int n_extra);
int i3d_hardneg_loss_fwd(int mode, const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim, int pos_offset,
                         int norm, double tau, double tau_plus, double beta, double extra_weight, double loss_scale, float* scratch,
                         float* loss, void* stream);
int i3d_hardneg_loss_bwd(int mode, const float* z1, const float* z2, const float* x, int b1, int b2, int n_extra, int dim, int pos_offset,
                         int norm, double tau, double beta, double loss_scale, const float* scratch, const float* grad_scale_dev,
                         float* work, float* dz1, float* dz2, float* dx, void* stream);

/* ---- the non-contrastive objectives (csrc/batchstat.hip; reference commons/losses.py BarlowTwinsLoss :45-73, CosineSimilarityLoss
 * :76-95, RegularizationLoss :98-123, CriticLoss :33-42, std_loss / cov_loss :954-964) ----
 * fp32 in and out; every sum fp64 in a fixed order, no atomics; nothing synchronises with the host.
 * Column family, z1, z2 [n, dim] (z2 null: one view), n >= 2:
 * i3d_bs_moments: mom [views, 2, dim] (fp64) = the column means and the unbiased variances sum_i (z_ij - mean_j)^2 / (n - 1), the mean
 *   first, then the centred squares; a1, a2 (null: not written) = (z - mean) / std with no epsilon, c1, c2 (null: not written) =
 *   z - mean; both views in one launch of 16-column workgroups.
 * i3d_bs_matrix_pass: m [count, dim, dim], with C = m inv_n: partial [count, i3d_bs_pass_blocks(dim)] (fp64) = each workgroup's share of
 *   w_diag sum_i (C_ii - target)^2 + w_off sum_{i != j} C_ij^2, and m is overwritten with G = d(that sum)/dC (w_diag == 0: the diagonal
 *   is not read into the sum and G_ii = 0).  BarlowTwins: m = a1^T a2, inv_n = 1 / n, target 1, w_diag = scale_loss, w_off = scale_loss
 *   lambd.  Covariance term: m = c^T c, inv_n = 1 / (n - 1), w_diag = 0, w_off = weight / dim.
 * i3d_bs_finish: loss[0] = scale sum(partial[0 .. n_partial)) + var_w / dim sum_{view, j} relu(1 - sqrt(var_j + 1e-4)) over mom (var_w
 *   == 0: mom is not read); one workgroup.
 * i3d_bs_col_bwd: dz = g [sa (da - colmean(da) - a colsum(da a) / (n - 1)) / std + sc (dc - colmean(dc)) + hc_j (z - mean_j)] for both
 *   views in one launch; da = a_other G^(T) and dc = c G come from the GEMM (null: the term is absent; BarlowTwins sa = 1 / n, covariance
 *   sc = 2 / (n - 1) since its G is symmetric), hc_j = -var_w / (dim (n - 1) sqrt(var_j + 1e-4)) where the hinge is active, g =
 *   grad_scale grad_scale_dev[0] (null: 1).  dz2 null: one view.
 * Row family, x [rows, dim], y [rows, dim, reps] (element (b, d, r) at (b dim + d) reps + r), reps in 1..i3d_bs_max_repeats() = 32:
 * i3d_bs_rows_fwd: rowloss [rows] (fp64) = sum_r sum_d (x_d / max(|x|, 1e-12) - y_dr / max(|y_r|, 1e-12))^2, stats [rows, 1 + 2 reps]
 *   (fp64) = |x|, |y_r|, <x, y_r>; one workgroup per row, y read in memory order.  The mean is i3d_bs_finish with scale = 1 / (rows reps).
 * i3d_bs_rows_bwd: dx [rows, dim], dy [rows, dim, reps] of grad_scale grad_scale_dev[0] sum_b rowloss_b in one launch; a norm below
 *   1e-12 keeps the constant denominator (torch F.normalize). */
int i3d_bs_max_repeats(void);
int i3d_bs_pass_blocks(int dim);
int i3d_bs_moments(const float* z1, const float* z2, int n, int dim, float* a1, float* a2, float* c1, float* c2, double* mom,
                   void* stream);
int i3d_bs_matrix_pass(float* m, int count, int dim, double inv_n, double target, double w_diag, double w_off, double* partial,
                       void* stream);
int i3d_bs_finish(const double* partial, int n_partial, double scale, const double* mom, int views, int dim, double var_w, float* loss,
                  void* stream);
int i3d_bs_col_bwd(const float* z1, const float* z2, const float* a1, const float* a2, const float* da1, const float* da2,
                   const float* dc1, const float* dc2, int n, int dim, const double* mom, double sa, double sc, double var_w,
                   double grad_scale, const float* grad_scale_dev, float* dz1, float* dz2, void* stream);
int i3d_bs_rows_fwd(const float* x, const float* y, int rows, int dim, int reps, double* stats, double* rowloss, void* stream);
int i3d_bs_rows_bwd(const float* x, const float* y, int rows, int dim, int reps, const double* stats, double grad_scale,
                    const float* grad_scale_dev, float* dx, float* dy, void* stream);

/* ---- SAN: the edge attention of the spectral-attention baseline (reference models/san.py:111-177; csrc/san.hip) ----
 * N = num_nodes >= 0, E = num_edges >= 0, H = feat >= 1, nh = heads >= 1 with H % nh == 0, V = num_codes >= 1; anything else returns
 * I3D_ERR_INVALID before a launch.  The kernels cover dh = H / nh <= 64, nh G <= 512 (G the power of two >= max(dh, 4)) and V <= 256;
 * every other valid call returns I3D_NOT_TAKEN (i3d_san_attn_takes answers the same without pointers) and the caller composes the
 * step.  N = 0 returns I3D_OK without a launch.
 * q, k, v, q2, k2 [N, H] with leading dimension ld (column blocks of one [N, 5H] product); te, te2 [V, H] contiguous: the edge
 * projections E(e), E_2(e) of every bond-feature combination; codes [E] (i3d_edge_codes) and real [E] (0 / 1) in destination-sorted
 * order (graph.GraphIndex).  full_graph == 0: every edge is real with coefficient 1 and q2, k2, te2, real, dq2, dk2, dte2 are ignored.
 * i3d_san_attn_fwd: s[p, a] = sum_{d in head a} Ksel_src[d] Qsel_dst[d] Tsel[codes[p]][d] / sqrt(dh)  [E, nh] with (k, q, te) on a real
 *   edge and (k2, q2, te2) on a fake one; w = exp(clamp(s, -5, 5)) coef, coef = 1 / (gamma + 1) real, gamma / (gamma + 1) fake;
 *   z[i, a] = sum over the in-edges of w  [N, nh];  out[i, d] = sum over the in-edges of w V_src[d] / (z[i, a] + 1e-6)  [N, H]
 *   contiguous, an exact zero row for a node without in-edges.  One launch, one wave per destination.
 * i3d_san_attn_bwd: from g = dL/dout [N, H] and the forward's out, z, s: dq, dk, dv, dq2, dk2 [N, H] with leading dimension ldg
 *   (dk, dk2, dv gathered over the out-edges in out_ptr / out_epos order), dte, dte2 [V, H] summed in fp64 over chunks of
 *   i3d_san_attn_chunk_edges() positions of the code-sorted edge list (code_order, code_ptr: ops.code_sorted_index), then per code
 *   over its chunks (four quarters, each in chunk order, then the four in order), a zero row for a code without edges.  No gradient flows through a score outside [-5, 5].  Scratch: gn [N, H],
 *   ds [E, nh], partials of i3d_san_attn_bwd_partial_floats(E, H, V) floats, 8-byte aligned.  Four launches (three when E = 0); fixed
 *   summation order, no atomics, no [E, H] buffer in either direction. */
/* i3d_san_edge_codes: codes[p] = sum_c feat[perm[p], c] strides[c] (int32) and real[p] = real_in[perm[p]] != 0 (uint8) for every edge
 *   position p of the destination-sorted order; feat [E, n_cols] and real_in [E] int64 in edge-id order, strides a host array,
 *   n_cols in 1..8; real_in and real both null: no flags.  One launch, none for E = 0. */
int i3d_san_edge_codes(const int64_t* feat, const int64_t* real_in, const int* perm, int num_edges, int n_cols, const int* strides,
                       int* codes, unsigned char* real, void* stream);
int i3d_san_attn_chunk_edges(void);
int i3d_san_attn_takes(int feat, int heads, int num_codes);
long i3d_san_attn_bwd_partial_floats(int num_edges, int feat, int num_codes);
int i3d_san_attn_fwd(const float* q, const float* k, const float* v, const float* q2, const float* k2, int ld, const float* te,
                     const float* te2, int num_codes, const int* codes, const unsigned char* real, const int* in_ptr,
                     const int* src_s, int num_nodes, int num_edges, int feat, int heads, int full_graph, float gamma, float* out,
                     float* s, float* z, void* stream);
int i3d_san_attn_bwd(const float* g, const float* out, const float* z, const float* s, const float* q, const float* k, const float* v,
                     const float* q2, const float* k2, int ld, const float* te, const float* te2, int num_codes, const int* codes,
                     const unsigned char* real, const int* in_ptr, const int* src_s, const int* dst_s, const int* out_ptr,
                     const int* out_epos, const int* code_order, const int* code_ptr, int num_nodes, int num_edges, int feat,
                     int heads, int full_graph, float gamma, float* gn, float* ds, float* partials, float* dq, float* dk, float* dv,
                     float* dq2, float* dk2, int ldg, float* dte, float* dte2, void* stream);

/* ---- SMP / SphereNet: geometry, raw bases and the triplet interaction (reference models/spherical_message_passing.py,
 * commons/spherical_encoding.py; csrc/smp.hip) ----
 * N = num_nodes, B = num_graphs, E = num_edges, T = num_triplets, all >= 0; n = num_spherical in 1..7, k = num_radial in 1..64,
 * I = int_emb >= 1, Bs = basis_emb >= 1; anything else returns I3D_ERR_INVALID before a launch.  A zero count returns I3D_OK without
 * a launch wherever nothing is to be written.
 * pos [N, 3] fp32, mol [N] the molecule of every atom (non-decreasing), graph_ptr [B + 1] the atoms of every molecule.
 * i3d_smp_radius_count: deg[i] = min(i3d_smp_max_neighbors(), atoms j != i of i's molecule with |pos_i - pos_j|^2 < cutoff^2 in fp32).
 * i3d_smp_radius_fill: with in_ptr [N + 1] the exclusive prefix sum of deg, the edges j -> i at in_ptr[i].., sources ascending - the
 *   lowest indices within range when the cap cuts, so j -> i may exist without i -> j -: src, dst [E], dist [E] (differences, squares, sum
 *   and root in fp64 from the fp32 positions, rounded once).
 * i3d_smp_triplet_count: count[e] = in-edges (k -> j) of the source j of e = (j -> i) with k != i.
 * i3d_smp_triplet_fill: with trip_ptr [E + 1] the prefix sum of count: idx_kj[t] the position of (k -> j), idx_ji[t] = e, grouped by e,
 *   k ascending inside a group - the order of the reference's xyztodat.
 * i3d_smp_bases: angle, torsion [T] (xyztodat's expressions in fp64, rounded once; the candidate k_n == k of the torsion minimum is set
 *   to 2 pi, not computed) and the raw bases sbf [T, n k], t [T, n n k] of angle_emb / torsion_emb: no envelope, the real harmonics per
 *   l as [m = 0, cos m = 1..l, sin m = l..1], flat harmonic f paired with the Bessel order f % n.  zeros, norm [n, k] and pref [n n]
 *   fp64: the fp32-rounded Bessel zeros, the normalisers from them and the harmonics' prefactors (sqrt 2 folded in for m > 0), built by
 *   the host.  Bessel functions by series / upward recurrence in fp64.  Scratch: rbf_ws [E, n k], cbf_ws [T, n n] fp64.  Three launches.
 * Triplet interaction: out[e, c] = sum_{t in group e} x[idx_kj[t], c] (sum_b w1[c, b] s8[t, b]) (sum_b w2[c, b] t8[t, b]) with x [E, I],
 *   s8, t8 [T, Bs], w1, w2 [I, Bs] contiguous.  The kernels cover I <= 256 and Bs <= 8; every other valid shape returns I3D_NOT_TAKEN
 *   (i3d_smp_triplets_takes answers the same without pointers) and the caller composes the step.
 * i3d_smp_triplets_fwd: one launch, one wave per ji edge; an edge without triplets gets an exact zero row.
 * i3d_smp_triplets_bwd (E, T >= 1): from g = dL/dout [E, I]: ds8, dt8 [T, Bs] (wave per ji edge), dx [E, I] gathered over the kj-grouped
 *   list (kj_ptr [E + 1], kj_order [T]: the triplets sorted stably by idx_kj), dw1, dw2 [I, Bs] summed in fp64 over chunks of
 *   i3d_smp_triplets_chunk() triplets, then per element over the chunks (four quarters, each in chunk order, then the four in order).
 *   Scratch: partials of i3d_smp_triplets_bwd_partial_floats(T, I, Bs) floats, 8-byte aligned.  Four launches; fixed summation order, no
 *   atomics, no [T, I] buffer in either direction. */
int i3d_smp_max_neighbors(void);
int i3d_smp_radius_count(const float* pos, const int* mol, const int* graph_ptr, int num_nodes, int num_graphs, float cutoff, int* deg,
                         void* stream);
int i3d_smp_radius_fill(const float* pos, const int* mol, const int* graph_ptr, const int* in_ptr, int num_nodes, int num_graphs,
                        int num_edges, float cutoff, int* src, int* dst, float* dist, void* stream);
int i3d_smp_triplet_count(const int* src, const int* dst, const int* in_ptr, int num_edges, int* count, void* stream);
int i3d_smp_triplet_fill(const int* src, const int* dst, const int* in_ptr, const int* trip_ptr, int num_edges, int num_triplets,
                         int* idx_kj, int* idx_ji, void* stream);
int i3d_smp_bases(const float* pos, const float* dist, const int* src, const int* dst, const int* in_ptr, const int* idx_kj,
                  const int* idx_ji, int num_edges, int num_triplets, int num_spherical, int num_radial, float cutoff,
                  const double* zeros, const double* norm, const double* pref, double* rbf_ws, double* cbf_ws, float* angle,
                  float* torsion, float* sbf, float* t, void* stream);
int i3d_smp_triplets_takes(int int_emb, int basis_emb);
int i3d_smp_triplets_chunk(void);
long i3d_smp_triplets_bwd_partial_floats(int num_triplets, int int_emb, int basis_emb);
int i3d_smp_triplets_fwd(const float* x, const float* s8, const float* t8, const float* w1, const float* w2, const int* trip_ptr,
                         const int* idx_kj, int num_edges, int num_triplets, int int_emb, int basis_emb, float* out, void* stream);
int i3d_smp_triplets_bwd(const float* g, const float* x, const float* s8, const float* t8, const float* w1, const float* w2,
                         const int* trip_ptr, const int* idx_kj, const int* idx_ji, const int* kj_ptr, const int* kj_order,
                         int num_edges, int num_triplets, int int_emb, int basis_emb, float* partials, float* dx, float* ds8,
                         float* dt8, float* dw1, float* dw2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFOMAX3D_HIP_H */
