/*
 * spe_hip.h - C ABI of libspe_hip.so: the MI355X (gfx950) kernels behind the SPE hot path.
 *
 * The reference (MingXiangL/SPE) has no native code: every "kernel" on its hot path is an
 * implicit ATen/cuBLAS launch issued from Python.  Each entry point
 * below therefore cites the reference *Python* site whose device work it replaces.  The
 * Python host code in spe_amd/ binds these with ctypes (spe_amd/lib.py); INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (the kernels never allocate);
 *   - tensors are fp32, row-major, densely packed unless a leading dimension is passed;
 *   - `stream` is the hipStream_t the work is enqueued on; calls are asynchronous;
 *   - return value: 0 on success, a positive hipError_t on launch failure, a negative value
 *     for an unsupported argument combination; no exception crosses the boundary;
 *   - dropout masks are a pure function of (seed, offset, element index) - Philox4x32 with 7 rounds (csrc/common.h) -
 *     so forward and backward regenerate the same mask (the attention's backward loads the 1-bit keep flags its forward stored).
 */
#ifndef SPE_HIP_H
#define SPE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* spe_stream_t; /* == hipStream_t */

/* 2 since round 2 (changed signatures: spe_hungarian, spe_adamw_flat, spe_layernorm_fwd, spe_attn_contract,
 * spe_talking_fused_plan; new entry points); 3 since round 3 (fp16 forward formats of the fused attention: spe_attn_contract
 * takes `fmt`, spe_attn_pack_multi kinds carry an element-format bit, spe_talking_fused expects fp16 Q / K fragments and writes
 * fp16 P'd blocks; split-operand GEMM entry points); 4: deterministic reductions - spe_set_reduce_workspace is new and required
 * before any entry point that sums across workgroups, spe_box_loss takes L, spe_linear_small_fwd / _bwd are new; 5 (round 4):
 * the flash-style talking-heads entry points spe_talking_flash_* are new; 6 (round 5): spe_talking_bwdq_* are new; 7 (round 6): ONE attention
 * backward composition - spe_talking_fused(_bits / _plan), spe_attn_merge, spe_talking_flash_rows, spe_talking_flash_dv, spe_talking_bwdq_pass1 removed,
 * spe_talking_stats(_plan) new (the statistics pass alone), spe_rowdot new, spe_layernorm_res_bwd takes dy2.  Still 7 after purely additive
 * entry points: spe_conv_head_fwd / _plan / _bwd and spe_attn_pmean(_dense) (the woct0head backbones' conv class head and patch-affinity CAMs),
 * spe_gemm_bf16nt_plan / spe_gemm_bf16tn_plan (the kernel selection of the 16-bit NT GEMM family / of the TN weight-gradient GEMM, host only),
 * spe_pos_learned_fwd / _bwd (the learned position embedding), spe_cam_boxes_device(_workspace) (the CAM pseudo boxes found on the device), spe_voc_match / spe_voc_ap (VOC AP and CorLoc on the device),
 * spe_coco_match / spe_coco_accumulate (the COCO AP / AR tables on the device),
 * spe_resample_plan / _tables / _h / _v (the input transforms: Pillow-exact bilinear resize, crop, flip, normalise, pad),
 * spe_ledger_state_bytes / _record / _total_bwd / _summary (the step ledger: weighted total, loss meters and non-finite guard on the device)
 * spe_gemm_f32_plan (the kernel selection and launch choices of spe_gemm_f32 / spe_gemm_ex, host only)
 * spe_jpeg_probe / _entropy / _reconstruct (baseline JPEG decoding: host entropy pass, device IDCT to RGB)
 * spe_adamw_flat_ema / spe_swap_flat (the weight EMA kept inside the optimizer's update launch, and its exchange with the parameters)
 * spe_linear_small_plan (the launch choices of the spe_linear_small_* entries, host only)
 * spe_grad_report (per-parameter gradient and weight statistics on the flat buckets, gated on the guard block: what a skipped step skipped)
 * spe_cls_ap / spe_cls_ap_workspace (the multi-label classification AP of the image-label logits on the device)
 * spe_cam_targets / spe_refine_pick (the training targets assembled on the device: CAM boxes -> target rows, the stage k+1 picks in one launch)
 * spe_pseudo_quality (the quality of the pseudo labels against the loader's ground truth: per-class counters kept on the device)
 * spe_proposal_recall (recall-at-k and ceiling of a stage's Q query boxes against the loader's ground truth: per-class counters kept on the device)
 * spe_rowops_plan (the kernel and grid the column-sum, LayerScale, activation-backward and dropout launchers choose for a shape, host only)
 * - 117 entry points.  Still 7: spe_mha_bwd refuses nch > 1 without dq_ws (-2) instead of adding the chunks into dq atomically (no caller did). */
int spe_abi_version(void);

/* ---- reduction workspace --------------------------------------------------------------------
 * Every sum across workgroups on the gradient path (bias / LayerNorm gamma, beta / LayerScale gamma column sums of
 * spe_layernorm_bwd, spe_layernorm_res_bwd, spe_colsum, spe_cvt_bf16, spe_gemm_bf16nt_ex, spe_layerscale_residual_bwd(16), the
 * loss sums of spe_focal_loss; reference: the reductions autograd performs for models/cait.py:376-416, models/transformer.py:
 * 279-287 and models/conditional_detr.py:253-275) is taken in a FIXED order - per-workgroup partials in slabs, integer tickets, the
 * last arriver adds (csrc/det_reduce.h) - so gradients are bitwise reproducible run to run; no fp32 atomics.  The slabs and tickets
 * live in caller-owned device memory registered here once per process (256-B aligned, >= 2 MiB; 16 MiB covers every shape of
 * the model path); entry points that need it return -4 when none is registered or it is too small.  All launches that use it
 * must be ordered on one stream at a time.  ws = NULL unregisters. */
int spe_set_reduce_workspace(void* ws, size_t bytes, spe_stream_t stream);
/* Deferred sums (round 4).  The fixed-order tree costs the last workgroup of every launch six dependent trips to the coherence point
 * (5-8 us; ~250 launches per step).  When the destination of a sum is a parameter gradient inside the caller's all-reduce buckets, nothing
 * reads it before the bucket is reduced / the optimiser runs: the owner of the buckets registers their address ranges
 * (spe_reduce_defer_ranges: n <= 64 ranges, n = 0 switches deferral off) and an arena (spe_reduce_defer_arena: caller-owned device memory,
 * 256-B aligned, a few tens of MB); entry points whose destinations ALL lie inside the ranges (spe_layernorm_bwd / _res_bwd,
 * spe_layerscale_residual_bwd16(d), spe_cvt_bf16 with colsum, spe_gemm_bf16nt_ex(d) with colsum, spe_colsum_bf16_blocks) then only leave
 * their per-workgroup partial rows in the arena, and spe_reduce_flush adds the rows of ALL pending launches to their destinations in ONE
 * kernel (members in index order: bitwise reproducible), stream-ordered after them.  The caller MUST flush before anything reads those
 * gradients (before a bucket's all-reduce, at the end of the backward); the library flushes by itself when its table or the arena is full.
 * spe_reduce_pending: launches waiting for a flush.  -3: ranges / arena changed while sums are pending. */
int spe_reduce_defer_ranges(const void* const* ptrs, const size_t* bytes, int n);
int spe_reduce_defer_arena(void* arena, size_t bytes);
int spe_reduce_flush(spe_stream_t stream);
int spe_reduce_pending(void);

/* ---- contraction ----------------------------------------------------------------------
 * C[z] = act(alpha * opA(A[z]) @ opB(B[z]) + bias) for z = (z0, z1) in batch0 x batch1, each
 * operand addressed as base + z0*s?0 + z1*s?1.  transA=0: A is [M,K] (lda); transA=1: A is
 * [K,M].  transB=0: B is [K,N] (ldb); transB=1: B is [N,K] (nn.Linear weight layout).
 * act: 0 none, 1 ReLU, 2 exact-erf GELU; C2 (optional) receives the pre-activation.
 * splitk>1: K is split over workgroups and atomically accumulated into a PRE-ZEROED C
 * (bias/act/C2 must be null/0).  splitk<-1: |splitk| splits, split z stores its partial result into the
 * private slab C + z*S (no atomics); the caller sums the slabs (spe_colsum over |splitk| rows of S floats), S = M*ldc
 * for a single matrix, else the extent of the batched C: ((batch0-1)*sC0 + (batch1-1)*sC1 + (M-1)*ldc + N) rounded up to 4.  precision: 0 = bf16 MFMA operands, fp32 accumulate;
 * 1 = 3-term bf16 split (~fp32 accuracy).
 * Replaces nn.Linear / torch.bmm / `@` at reference models/cait.py:376-390 (qkv, QK^T, PV, proj),
 * :114-133 (class attention), timm Mlp fc1/fc2 (cait.py:409), Conv2d patch embed (cait.py:526),
 * models/transformer.py:368-425 (decoder projections, FFN), models/attention.py:353,375,378,
 * models/conditional_detr.py:104-110 (heads), and every one of their autograd backward GEMMs. */
int spe_gemm_f32(const float* A, const float* B, float* C, const float* bias, float* C2,
                 int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB,
                 int batch0, int batch1, long sA0, long sA1, long sB0, long sB1, long sC0, long sC1,
                 float alpha, int act, int splitk, int precision, spe_stream_t stream);

/* Same contraction with the A operand stored as bf16 when a_bf16 = 1 (lda and sA0/sA1 count bf16
 * elements): consumes the transposed score tensors written by spe_talking_fused for the PV / dV /
 * dQ / dK products of reference models/cait.py:389 and its autograd. */
int spe_gemm_ex(const void* A, int a_bf16, const float* B, float* C, const float* bias, float* C2,
                int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB,
                int batch0, int batch1, long sA0, long sA1, long sB0, long sB1, long sC0, long sC1,
                float alpha, int act, int splitk, int precision, spe_stream_t stream);

/* Tile edge (128 or 64) spe_gemm_* will use for an (M, N, batch) problem; callers use it to choose split-K. */
int spe_gemm_tile(int M, int N, int nbatch);
/* spe_gemm_f32_plan: which instance of spe_gemm_kernel<T, TA, TB, SPLIT> spe_gemm_f32 / spe_gemm_ex run for a problem and every launch
 * choice that goes with it.  Host only: no device, no stream, nothing is launched; the launcher calls the same function, so tests and
 * tools can tell which kernel and which load / tile-order path a shape exercises.  The arguments are those of spe_gemm_ex that influence
 * the choice; epilogue = 1 when a bias, an activation or C2 is asked for; a_mod16 / b_mod16 are the addresses of A / B modulo 16.
 * v[11] = { T (tile edge), TA, TB, SPLIT, splitk (effective: a request above the number of 32-wide k-tiles is clamped to it), kt_per_split
 * (k-tiles per split; the last splits may get fewer, or none), slab (floats between the slabs of a splitk < 0 launch, else 0), vecA, vecB
 * (16-byte operand loads: base aligned - 8 bytes for a bf16 A - and leading dimension and batch strides multiples of 4), xcd_bind (0 plain
 * tile order, 1 / 2: M / N panels bound to XCDs), grid.x (tiles plus padding workgroups) }; all zero when M, N or a batch count is <= 0
 * (nothing to do).  Returns the status spe_gemm_ex would return: -4 (K <= 0), -2 (transA and transB), -5 (more slabs than k-tiles), -3
 * (splitk > 1 with an epilogue), else 0. */
int spe_gemm_f32_plan(int M, int N, int K, long lda, long ldb, long ldc, int transA, int transB, int batch0, int batch1,
                      long sA0, long sA1, long sB0, long sB1, long sC0, long sC1, int splitk, int precision, int a_bf16,
                      int epilogue, int a_mod16, int b_mod16, long* v);

/* ---- LayerNorm (nn.LayerNorm; reference models/cait.py:403,407 eps 1e-6,
 * models/transformer.py:264-265,342-344 eps 1e-5).  C % 4 == 0, C <= 1024.
 * bwd: dgamma/dbeta are ACCUMULATED into (pre-zeroed or running) buffers; add (optional, [R][C]; may alias dx) is added to
 * dx - the gradient arriving over the residual path around the normalised branch (x feeds both: cait.py:404-405), which
 * autograd would otherwise sum with one more elementwise launch.
 * fwd: y16 (optional, bf16 [R][C]): the same result rounded to bf16 - the operand of the Linear that consumes y, written by
 * the same pass instead of by a separate spe_cvt_bf16 launch; y16lo (optional, needs y16): bf16(y - bf16(y)), the low part of
 * the SPLIT operand of precision mode bf16s (see spe_gemm_bf16nt). */
int spe_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                      float* rstd, long R, int C, float eps, void* y16, void* y16lo, spe_stream_t stream);
/* spe_layernorm_fwd_h (round 5): the same, with the second 16-bit copy yh16 = IEEE fp16(y) (saturating) instead of the low part - the
 * operand of a single-term fp16 forward product (the backbone MLP's fc1 in precision mode bf16s); y16 stays the backward's bf16 operand. */
int spe_layernorm_fwd_h(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                        float* rstd, long R, int C, float eps, void* y16, void* yh16, spe_stream_t stream);
int spe_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                      const float* rstd, float* dx, float* dgamma, float* dbeta, long R, int C,
                      const float* add, spe_stream_t stream);
/* spe_layernorm_bwd_ls (round 5): spe_layernorm_bwd plus, in the same pass, the LayerScale backward of the node that CONSUMES dx - in a
 * backbone block the input of a norm is out = res + ls_gamma * ls_y, the output of the previous branch's Linear (reference models/cait.py:
 * 404-405), so dx is that node's `dout`: ls_dy16 [R][C] = bf16(ls_gamma * dx) (the operand of that Linear's backward GEMMs), ls_db[c] += sum_r
 * ls_gamma[c] dx[r][c] (its bias gradient), ls_dg[c] += sum_r dx[r][c] ls_y[r][c] (the LayerScale gradient) - what
 * spe_layerscale_residual_bwd16 computes from dx in a launch of its own.  ls_y fp32 [R][C]; no dropout / DropPath in that branch; C <= 512.
 * The caller must know that dx has no other consumer (the sums land in the gradients before the consuming node runs). */
int spe_layernorm_bwd_ls(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                         float* dgamma, float* dbeta, long R, int C, const float* add, const float* ls_y, const float* ls_gamma,
                         void* ls_dy16, float* ls_db, float* ls_dg, spe_stream_t stream);

/* ---- bf16-operand Linear GEMM (benchmark precision mode): C = act(alpha * A16 B16^T + bias), both operands
 * k-contiguous bf16 (lda, ldb, K multiples of 8; 16-B aligned bases), fp32 C / C2 (pre-activation) / bias.
 * splitk < 0: |splitk| K-slices write private slabs C + z*M*ldc (no bias/act; sum them with spe_colsum).
 * The three products of nn.Linear and its autograd (reference models/cait.py:376,390,409;
 * models/transformer.py:368-425) are NT products of copies made by spe_cvt_bf16:
 *   y = x W^T: (x16, W16) ; dx = dy W: (dy16, W16T) ; dW = dy^T x: (dy16T, x16T), contraction zero padded.
 * spe_cvt_bf16: out[R][ldo] = bf16(x) (round to nearest even, the rounding spe_gemm_f32 applies while staging)
 * and/or outT[C][ldt] = transpose, columns R..ldt-1 zero filled; colsum[c] += sum_r x[r][c] (fp32; the bias gradient
 * of the Linear, from the same read).  Any of the three outputs may be NULL.  Alignment: x and aux need only their 4 bytes (rows are
 * read as 16-byte vectors when ldx % 4 == 0 and x is 16-byte aligned, element by element otherwise); out / out_lo must be 8-byte aligned
 * when ldo % 4 == 0 and outT when ldt % 4 == 0 (quads are then stored as 8-byte vectors; any other ldo / ldt: 2-byte stores, 2-byte
 * alignment) - a column block of a wider bf16 matrix therefore starts at a column that is a multiple of 4.  ldt may exceed R by any
 * amount: all of columns R..ldt-1 are zero filled.  Measured on the MI355X (tests/test_cvt16_gpu.py, profiles/cvt16_edges.txt): fp32
 * subnormal inputs are converted like any other value - the bf16 copy keeps them as bf16 subnormals, rounded to nearest even, and
 * the low part is bf16(x - bf16(x)) of them as well; nothing is flushed to zero.  aux != NULL: x is first multiplied by the
 * activation derivative at aux (act 1: ReLU with aux = forward output, 2: erf-GELU with aux = pre-activation; same
 * layout and leading dimension as x) - the backward of a fused Linear+activation without an fp32 intermediate.
 * SPLIT operands (precision mode "bf16s", the forward products): A16lo / B16lo (both or neither; same leading dimensions as
 * A16 / B16) hold bf16(x - bf16(x)) of the fp32 operands, written next to the high parts by every producer (out_lo of
 * spe_cvt_bf16 / spe_cvt_bf16_multi, y16lo of spe_layernorm_fwd, out16lo of spe_attn_contract and spe_gemm_bf16nt_ex); the
 * product is then A_hi B_hi + A_lo B_hi + A_hi B_lo - ~16 significant operand bits instead of 8 at 3x the MFMA work of kernels
 * that are load / store bound (no split-K with split operands).  * act bits 8 / 9 (round 4, the decoder's memory-side projections - north_star's "decoder cross-attention GEMM", reference
 * models/transformer.py:389-396): bit 8 = A16 / B16 hold IEEE fp16 and the product is single-term on v_mfma_f32_16x16x32_f16 (no lo
 * parts); bit 9 = C is an IEEE fp16 [M][ldc] matrix (saturating) - what spe_attn_pack_multi's fp16-source jobs consume.  Both need
 * splitk = 1, no C2, ldc % 4 == 0; bit 8 needs M >= 2048 and K % 64 == 0.  spe_cvt_f16: fp32 [R, C] -> IEEE fp16 (C, ldx, ldo % 4 == 0). */
int spe_cvt_f16(const float* x, long ldx, int R, int C, void* out, long ldo, spe_stream_t stream);
int spe_gemm_bf16nt(const void* A16, const void* B16, const void* A16lo, const void* B16lo, float* C, const float* bias,
                    float* C2, int M, int N, int K, long lda, long ldb, long ldc, float alpha, int act, int splitk,
                    spe_stream_t stream);
/* nn.Linear on a few hundred rows (the decoder / encoder / head side: reference models/transformer.py:21-33, 206-250, 355-427,
 * models/conditional_detr.py:68-116) as ONE launch each way - these products are bound by dependent launches, not by throughput.
 * spe_linear_small_fwd: y[R][ldc] = act(x W^T + bias) from the fp32 activations x [R][ldx] and the cached bf16 weight W16 [N][K]
 *   (W16lo != NULL: split operands, x is split into (hi, lo) while it is staged - precision mode bf16s); pre (optional): the
 *   pre-activation; x16_out (optional): bf16(x) [R][K], all the backward needs of x.  act: 0 none, 1 ReLU, 2 exact-erf GELU.
 * spe_linear_small_bwd: dx [R][K] = dy' W, dW [N][K] = dy'^T x, db [N] = colsum(dy') in one grid, dy' = dy (fp32 [R][N]) times
 *   the derivative of the fused activation at aux (act 1: forward output, act 2: pre-activation; aux NULL: none); x16 [R][K] and
 *   WT16 [K][N] bf16; any of dx / dW / db may be NULL.  dW and db are OVERWRITTEN (no zeroing needed), db is summed in a fixed
 *   order (no atomics).
 * Status -2 (nothing launched, nothing written) - forward: K <= 0 or no multiple of 8, ldx no multiple of 4, or x, W16, W16lo, x16_out not
 *   16-B aligned; N, ldc, y, pre and bias are free (an unaligned y / pre or ldc % 4 != 0 takes 4-byte stores).  Backward: K or N no
 *   multiple of 8; dy, aux, x16, WT16, dx or dW not 16-B aligned (db is free); dx without WT16, dW without x16, aux with an act other
 *   than 1 or 2.  R or N <= 0 (backward: or K <= 0): status 0, nothing to do - as when none of dx / dW / db is asked for. */
int spe_linear_small_fwd(const float* x, long ldx, const void* W16, const void* W16lo, const float* bias, float* y, float* pre,
                         void* x16_out, int R, int N, int K, long ldc, int act, spe_stream_t stream);
int spe_linear_small_bwd(const float* dy, const float* aux, int act, const void* x16, const void* WT16, float* dx, float* dW,
                         float* db, int R, int N, int K, spe_stream_t stream);
/* Group form (round 4): nblk Linears of equal shape [N][K] applied to ONE input - the decoder layer's query-side projections
 * (reference models/transformer.py:368-372: sa_qcontent / sa_kcontent / sa_v of tgt; 369-371, 399: sa_qpos / sa_kpos of every layer and
 * ca_qpos of the first on query_pos) - as one launch each way; every Linear keeps its own cached weight copies, output and gradient
 * buffers: the arguments are HOST arrays of nblk device pointers, nothing is stacked.  nblk <= 16.
 * spe_linear_small_group_fwd: y[i] [R][N] = x W_i^T + bias[i] (+ add[i], a contiguous fp32 [R][N]; `add` or single elements may be NULL - the
 *   decoder's q = sa_qcontent_proj(tgt) + sa_qpos_proj(query_pos), transformer.py:373-374, without an add launch) (W16lo != NULL: split operands, every
 *   element non-NULL); N % 32 == 0.
 * spe_linear_small_group_bwd: dx [R][K] = sum_i dy[i] W_i (WT16[i] = bf16 W_i^T [K][N]), dW[i] [N][K] = dy[i]^T x16, db[i] [N] =
 *   colsum(dy[i]), overwritten, fixed summation order; dy[i] == NULL: output i received no gradient - it adds nothing to dx and its
 *   dW[i] / db[i] are not written.  dx, dW, db (or single elements of dW / db) may be NULL.  N % 128 == 0. */
int spe_linear_small_group_fwd(const float* x, long ldx, const void* const* W16, const void* const* W16lo, const float* const* bias,
                               const float* const* add, float* const* y, void* x16_out, int R, int nblk, int N, int K, spe_stream_t stream);
/* Status -2 of the group entries - both: nblk > 16, K <= 0 or no multiple of 8.  Forward: N % 32, ldx % 4, x / x16_out / W16[i] / W16lo[i] / y[i] / add[i] not
 *   16-B aligned, a NULL W16[i] or y[i], a NULL W16lo[i] when W16lo is given (`bias` or single bias[i] may be NULL: no bias).  Backward:
 *   N % 128, x16 / dx / dy[i] / WT16[i] / dW[i] not 16-B aligned, dx without WT16 or with a NULL WT16[i], dW without x16.  R, N or nblk <= 0
 *   (backward: or K <= 0): status 0.  Backward with every dy[i] NULL: dx, if asked for, is all zeros, no dW / db is written. */
int spe_linear_small_group_bwd(const float* const* dy, const void* x16, const void* const* WT16, float* dx, float* const* dW,
                               float* const* db, int R, int nblk, int N, int K, spe_stream_t stream);
/* spe_linear_small_plan: the launch choices of the four entries above for a problem.  Host only: no device, no stream, nothing is launched;
 * the entries fill their launch from the same function, so tests and tools can tell which kernel instance and which grid a shape takes.
 * entry: 0 spe_linear_small_fwd, 1 _bwd, 2 _group_fwd, 3 _group_bwd; N is the width of ONE Linear, nblk and ldx are ignored where the
 * entry has none; split: W16lo given; want_dx / want_dw / want_db: the outputs asked for (entry 1; entry 3 reads want_dx only); any_dw
 * (entry 3): some output i has a dy[i] and a dW[i] or db[i].
 * v[7] = { KC (contraction chunk of the k-contiguous programs: 384 or 128), RC (row chunk of the dW program: 512 or 256, 0 forward),
 * SPLIT, tiles_dx, tiles_dw (workgroups of the two backward programs; 0 forward), grid.x, dynamic LDS bytes } - the instance is
 * linear_small_fwd_kernel<KC, SPLIT> or linear_small_bwd_kernel<KC, RC>; all zero when there is nothing to do.  Returns the status the
 * entry would return for these arguments, except for the parts of -2 that depend on pointers. */
int spe_linear_small_plan(int entry, int R, int N, int K, int nblk, long ldx, int split, int want_dx, int want_dw, int want_db,
                          int any_dw, long* v);
/* spe_gemm_bf16tn: C[m][n] = alpha * sum_r A16[r][m] * B16[r][n] - the weight gradient dW = dy^T x of a Linear (autograd of
 * reference models/cait.py:376,390,409, models/transformer.py:368-425) on ROW-MAJOR bf16 operands A16 [R, lda] (M columns)
 * and B16 [R, ldb] (N columns): the contraction runs over rows, the MFMA operands are formed by LDS transpose reads
 * (ds_read_b64_tr_b16), no transposed copies of x or dy exist.  splitk < 0: |splitk| private slabs of M*ldc floats over
 * the row range (sum them with spe_colsum).  Operands 16-B aligned; lda, ldb, M, N multiples of 8. */
int spe_gemm_bf16tn(const void* A16, const void* B16, float* C, int M, int N, int R, long lda, long ldb, long ldc,
                    float alpha, int splitk, spe_stream_t stream);
/* spe_gemm_bf16tn_plan: which instance of gemm_bf16tn_kernel<BM, BN> spe_gemm_bf16tn runs for a problem and how it divides the rows -
 * the weight gradients of reference models/cait.py:376,390,409 and models/transformer.py:368-425 (see above).  Host only: no device, no
 * stream, nothing is launched; the launcher calls the same function, so tests and tools can tell which kernel a shape exercises.
 * v[4] = { BM, BN, splits (grid z), rt_per_split (64-row tiles per split; the last splits may get fewer, or none) }; all zero when M or
 * N <= 0 (nothing to do).  Returns the status spe_gemm_bf16tn would return, except for the pointer-alignment part of -2: -2 (lda, ldb, M
 * or N no multiple of 8, splitk > 1), -4 (R <= 0), -5 (more splits than 64-row tiles), else 0. */
int spe_gemm_bf16tn_plan(int M, int N, int R, long lda, long ldb, int splitk, int* v);
/* spe_gemm_bf16nt_ex: the same product with an epilogue that feeds the NEXT GEMMs directly (no fp32 round trip, no
 * separate conversion launch):  v = alpha A16 B16^T + bias ; C2 = v (optional) ; v = act(v), or with aux != NULL
 * v = v * act'(aux) (aux [M][ldc]: act 1 = ReLU with the forward output, act 2 = erf-GELU with the pre-activation) ;
 * C = v (optional fp32) ; out16[M][ld16] = bf16(v) ; out16T[N][ld16t] = bf16(v)^T with columns M..ld16t-1 zero
 * (ld16t <= M rounded up to 64) ; colsum[n] += sum_m v.  Any output may be NULL.  res/rgamma != NULL (act 0, no aux):
 * the LayerScale residual of the block is applied by the epilogue, C = res[m][n] + rgamma[n] * v (res [M][ldc]), while C2
 * keeps v for the gamma gradient.  half_flags bit 0: C2 is stored as IEEE fp16 [M][ldc] (saturating) instead of fp32; bit 1: aux
 * holds IEEE fp16 [M][ldc] - the saved pre-activation of the MLP, of which only gelu'(.) is ever taken.  Used by the fused MLP of the
 * backbone block (reference models/cait.py:405-416 = timm Mlp fc1 -> GELU -> fc2 inside x + gamma_2 * mlp(norm2(x)), and its autograd).
 * half_flags bits 2 / 3 (round 5: that MLP's FORWARD products in precision mode bf16s; profiles/r05_error_budget.jsonl - fp16 operands in
 * fc1 + fc2 alone cost <= 2.6e-4 on every weighted loss key at cfg2 / cfg5 full depth): bit 2 = A16 / B16 hold IEEE fp16, the product is
 * single-term on v_mfma_f32_16x16x32_f16 (no low parts; M >= 2048, K % 64 == 0) ; bit 3 (needs bit 2) = out16lo receives IEEE fp16(v)
 * (saturating) - the operand of the NEXT fp16 product - next to out16 = bf16(v), the backward's operand. */
int spe_gemm_bf16nt_ex(const void* A16, const void* B16, const void* A16lo, const void* B16lo, float* C, const float* bias,
                       float* C2, void* out16, void* out16lo, long ld16, void* out16T, long ld16t, float* colsum, const float* aux,
                       const float* res, const float* rgamma, int M, int N, int K, long lda, long ldb, long ldc, float alpha, int act,
                       int half_flags, spe_stream_t stream);
/* spe_gemm_bf16nt_exd (round 4): spe_gemm_bf16nt_ex with the backbone block's training rates inside the epilogue (reference models/cait.py:
 * 390-391 proj_drop, timm Mlp drop after GELU and after fc2, :404-416 drop_path): after the activation (or its derivative) v is multiplied
 * by the dropout keep scale of element m * N + n - the (seed, offset) stream of spe_dropout on the row-major [M][N] result, N % 4 == 0 - and
 * with res the epilogue writes C = res + sample_scale[m / rows_per_sample] * rgamma * v (sample_scale NULL: 1).  C2 keeps the RAW v: the
 * backward (spe_layerscale_residual_bwd16d) applies the same mask and scale. */
int spe_gemm_bf16nt_exd(const void* A16, const void* B16, const void* A16lo, const void* B16lo, float* C, const float* bias,
                        float* C2, void* out16, void* out16lo, long ld16, void* out16T, long ld16t, float* colsum, const float* aux,
                        const float* res, const float* rgamma, int M, int N, int K, long lda, long ldb, long ldc, float alpha, int act,
                        int half_flags, float p_drop, uint64_t seed, uint64_t offset, const float* sample_scale, long rows_per_sample,
                        spe_stream_t stream);
/* spe_gemm_bf16nt_plan: which kernel instance spe_gemm_bf16nt (ex = 0) / spe_gemm_bf16nt_ex(d) (ex = 1) run for a problem - the nn.Linear
 * products of reference models/cait.py:376,390,409 and models/transformer.py:368-425, 389-396 (see above).  Host only: no device, no
 * stream, nothing is launched; the launcher calls the same function (csrc/gemm_nt_select.h), so tests and tools can tell which kernel a
 * shape exercises.  split: A16lo / B16lo given; f16_operands: act bit 8 / half_flags bit 2; f16_second: half_flags bit 3; splitk as passed
 * to spe_gemm_bf16nt (1, or -n slabs); has_out16t / ld16t: the transposed copy of the extended epilogue.
 * plan[9] = { family (0: gemm_nt2_kernel - LDS-DMA ring, >= 2048 rows; 1: gemm_bf16nt_kernel - register-pipelined), BM, BN, BK,
 * NST (ring stages; family 1: 0), NTS (family 1: K tiles in flight at once, 0 = pipelined loop), SPLIT, EX, F16 }.
 * Returns the negative status the GEMM entry would return when no kernel covers the problem (-2), else 0. */
int spe_gemm_bf16nt_plan(int M, int N, int K, int split, int ex, int f16_operands, int f16_second, int splitk, int has_out16t,
                         long ld16t, int* plan);
int spe_cvt_bf16(const float* x, long ldx, int R, int C, void* out, void* out_lo, long ldo, void* outT, long ldt, float* colsum,
                 const float* aux, int act, spe_stream_t stream);
/* spe_cvt_bf16_h (round 5): out = bf16(x), out_h = IEEE fp16(x) (saturating; same layout as out), outT as above - one pass. */
int spe_cvt_bf16_h(const float* x, long ldx, int R, int C, void* out, void* out_h, long ldo, void* outT, long ldt, spe_stream_t stream);
/* spe_cvt_bf16_multi: the row-major and transposed bf16 copies of njobs contiguous fp32 matrices in ONE launch (every
 * Linear weight after an optimizer step).  jobs_dev: device array of njobs records of 64 bytes
 *   { const float* x; void* out; void* outT; long ldt; int R, C, tile0, tiles_c; void* out_lo; long flags; }     out, out_lo [R][C], outT [C][ldt], ldt >= R;
 * tiles_c = ceil(C/64), tile0 = running sum of tiles_c * ceil(max(R, ldt)/64) over the preceding jobs; total_tiles = that
 * sum over all jobs.  out, out_lo or outT may be NULL per job.  flags bit 0: out_lo receives IEEE fp16(x) instead of the low part.
 * Alignment as for spe_cvt_bf16 with ldx = ldo = C: out / out_lo 8-byte aligned when C % 4 == 0, outT when ldt % 4 == 0. */
int spe_cvt_bf16_multi(const void* jobs_dev, int njobs, int total_tiles, spe_stream_t stream);

/* ---- masked softmax over scores[B,H,Nq,ld] (Nk valid columns per row).
 * mask[B,Nk] (1 = padded key, -inf) or null; P = softmax; Pd = dropout(P) written only when
 * p_drop > 0.  Reference models/attention.py:363-373, models/cait.py:125-131 (class attention).
 * bwd: dS = P*(dP - sum dP*P) with dP = dPd*keepscale; dS may alias dPd. */
int spe_softmax_fwd(const float* S, const unsigned char* mask, float* P, float* Pd, int B, int H, int Nq,
                    int Nk, long ld, float p_drop, uint64_t seed, uint64_t offset, spe_stream_t stream);
int spe_softmax_bwd(const float* dPd, const float* P, float* dS, int B, int H, int Nq, int Nk, long ld,
                    float p_drop, uint64_t seed, uint64_t offset, spe_stream_t stream);

/* ---- talking-heads score transform (reference models/cait.py:379-387):
 * S' = proj_l(S) over heads, P = softmax_k(S'), P' = proj_w(P), Pd = attn_drop(P').
 * H in {4,6,8}.  P may alias S.  bwd consumes dPd, saved P and re-computed raw scores S and
 * writes dS (may alias dPd) plus `nblocks` rows of partial [dWl | dbl | dWw | dbw] sums
 * (row length 2*(H*H+H)) into ws; the caller column-sums ws (spe_colsum).  nblocks <= B*Nq. */
int spe_talking_softmax_fwd(const float* S, const float* Wl, const float* bl, const float* Ww, const float* bw,
                            float* P, float* Pd, int B, int H, int Nq, int Nk, long ld, float p_drop,
                            uint64_t seed, uint64_t offset, spe_stream_t stream);
int spe_talking_softmax_bwd(const float* dPd, const float* P, const float* S, const float* Wl, const float* Ww,
                            float* dS, float* ws, int nblocks, int B, int H, int Nq, int Nk, long ld,
                            float p_drop, uint64_t seed, uint64_t offset, spe_stream_t stream);

/* ---- fused talking-heads attention (reference models/cait.py:377-389 + autograd): qkv -> softmax(proj_l(scale q k^T)) -> proj_w -> attn_drop -> @ v
 * with NO N x N tensor in HBM for the forward (the backward's dS is the only one, bf16).  ONE composition:
 *   forward : spe_attn_pack_multi -> spe_talking_stats -> spe_attn_merge_rows -> spe_talking_flash_fwd
 *   backward: spe_attn_pack_multi(dO) -> spe_talking_bwdk_pass1 (D, dWw, dbw, dV) -> spe_talking_bwdq_pass2 (dS, dWl, dbl, dQ)
 *             -> spe_talking_wgrad_reduce -> spe_attn_contract(trans = 1) (dK)
 * (rounds 1-5 carried four backward compositions behind a developer switch - spe_talking_fused modes 1-3, spe_talking_fused_bits, spe_attn_merge,
 * spe_talking_flash_rows, spe_talking_flash_dv, spe_talking_bwdq_pass1; ABI 7 removed them: profiles/HISTORY_r05.md.)
 *
 * Operand format.  spe_attn_pack / spe_attn_pack_multi write 16-bit MFMA operand fragment records, per (b, h, 16-row tile):
 *   FULL steps of [lane][8] = scale * x[b, tile*16 + (lane&15), h, st*32 + (lane>>4)*8 + i], then - when dh % 32 is in
 *   1..16 - one 16-wide tail step of [lane][4] = scale * x[.., FULL*32 + (lane>>4)*4 + i]   (dh = 48: 1.5 KB/record)
 * from x[b][n][h][d] (element strides sb, sn, sh).  Qf and Kf are FP16 records (spe_attn_pack_multi kinds 0 + 16; Qf packed with scale * log2(e):
 * the kernels work in the log2 domain), Vf and dOf BF16 (kind 0): the forward quantities are O(1) and take the 3 extra mantissa bits, gradients
 * keep bf16's range.  Blocked score tensors (dS): bf16 16 x 16 blocks [B,H,nt,nt][64][4], nt = ceil(N/16), lane l of block (qt,kt) = query
 * qt*16+(l&15), keys kt*16+4*(l>>4)+i.
 *
 * spe_talking_stats: partial softmax statistics (running max, sum of exp2) of S' = proj_l(scale q k^T) per (b, g, q) -> ws_stats
 *   (B*nt*8*H*32 floats); spe_talking_stats_plan: the launcher's work split for an `nwg` workgroup budget (workgroups walk (q-tile pair, key tile)
 *   steps) - steps per workgroup (the value spe_attn_merge_rows needs) and workgroups used.
 * spe_attn_merge_rows: merges ws_stats into M (log2-domain row max), IL (1 / row sum) [B,H,N] and the row constants rows [B][Np][H] =
 *   bl[g] log2(e) - M + log2(IL), zero for the rows N .. Np-1 (the addend that turns Wl S into log2 P).  Np: multiple of 16, >= 16 ceil(N / 16).
 * spe_talking_wgrad_reduce: column sums of ws_w (nwg rows of 2*(H*H+H) = [dWl|dbl|dWw|dbw]) STORED (not accumulated) into the four gradient
 *   buffers in fixed order; a NULL destination is skipped.
 * Supported: H in {4,8}, head dim <= 64 and the LDS bounds below.  Returns -2 otherwise (use the materialised path: spe_talking_softmax_*).
 * spe_talking_fused_supported: 1 when the whole composition above runs for (H, head dim) - both are in the kernels' dispatch and the flash
 *   forward and the two backward kernels fit the LDS with attention dropout on - else 0 (an answer, not a status). */
int spe_talking_fused_supported(int H, int dh);
int spe_attn_pack(const float* x, long sb, long sn, long sh, int B, int N, int H, int dh, float scale,
                  void* out, spe_stream_t stream);
int spe_talking_stats_plan(int B, int N, int nwg, int* steps_per_wg, int* nwg_used);
int spe_talking_stats(const void* Qf, const void* Kf, const float* Wl, const float* bl, float* ws_stats,
                      int B, int H, int N, int dh, int nwg, spe_stream_t stream);
int spe_attn_merge_rows(const float* ws, float* M, float* IL, const float* bl, float* rows, int Np, int B, int H, int N,
                        int steps_per_wg, spe_stream_t stream);
int spe_talking_wgrad_reduce(const float* ws_w, int nwg, int H, float* dWl, float* dbl, float* dWw, float* dbw,
                             spe_stream_t stream);

/* ---- flash forward: P' goes from the head mix straight into the matrix instructions that consume it, the result accumulates in registers.
 * spe_talking_flash_plan: the launcher's flattened work split for an `nwg` workgroup budget (a workgroup keeps 8 tiles of 16 rows
 *   resident and streams the tiles of the other axis): steps per workgroup, workgroups launched, major tile groups per image, and
 *   Np = the padded row count of the row-constant arrays.  The partial-result workspace `ws` holds
 *   B * nmajor * 8 (slots) * 128 * H * 16 * ceil(dh / 16) floats.
 * spe_talking_flash_fwd: O[b, q, g*dh + d] = sum_key P'd[b,g][q,key] v[b, key, g, d] with P'd = attn_drop(proj_w(softmax(proj_l(
 *   scale q k^T)))); Qf / Kf fp16 fragments (spe_attn_pack_multi kind 0 + 16, Qf packed with scale * log2(e)), V16 fp16 (kind
 *   1 + 16), c0 = the row constants of spe_attn_merge_rows.  O16 / O16lo (optional): bf16(O) and bf16(O - bf16(O)), same addressing - the
 *   operand of the output projection.  keepbits (p_drop > 0 and a backward will follow): uint32 [B][nt][nt][64] - the dropout keep flags of
 *   every 16 x 16 tile (bit hp * 8 + 2 r + e of lane l: query l & 15, key 4 (l >> 4) + r, head 2 hp + e); the backward kernels LOAD them
 *   (one dword per lane and tile) instead of regenerating the masks.
 * Supported: H in {4, 8}, 13 * H * ceil(dh / 16) * 512 bytes of LDS (5 stage buffers + 8 resident tiles) <= 160 KB; -2 otherwise. */
int spe_talking_flash_plan(int B, int N, int nwg, int* steps_per_wg, int* nwg_used, int* nmajor, int* rows_padded);
int spe_talking_flash_fwd(const void* Qf, const void* Kf, const void* V16, const float* Wl, const float* Ww, const float* bw,
                          const float* c0, int Np, float* ws, float* O, void* O16, void* O16lo, void* keepbits, int B, int H, int N, int dh,
                          int nwg, float p_drop, uint64_t seed, uint64_t offset, spe_stream_t stream);

/* ---- the two backward kernels (reference: the autograd of models/cait.py:377-389 - proj_l, softmax, proj_w, attn_drop; csrc/attn_flash_bwd.hip).
 * A workgroup of 4 waves, ONE wave per SIMD (512 registers each): a wave keeps its tile's fragment records and 96 accumulators in AccVGPRs and
 * streams the tiles of the other axis through LDS.
 * spe_talking_bwdq_plan: the work split for an `nwg` workgroup budget - steps per workgroup, workgroups launched, major (4-tile) groups per
 *   image.  Workspaces: ws_q / ws_v B * nmajor * 8 * 4 * H * ceil(dh / 16) * 256 floats, ws_d B * nmajor * Np * H floats, ws_w
 *   (nwg_used * 4) rows of 2 * (H * H + H) floats - row layout [dWl | dbl | dWw | dbw], pass 2 fills the first half, pass 1 the second;
 *   spe_talking_wgrad_reduce(ws_w, 4 * nwg_used, ...) sums them.
 * spe_talking_bwdk_pass1 (KEY-major: a wave keeps one key tile's K / V records and 96 dV accumulators and streams the q-tiles): S, S', P recomputed
 *   ONCE for Drows[b][q][h'] = sum_key dP[h'] P[h'] ([B][Np][H], rows >= N zero; D summed over the 4 key tiles of a major in ws_d), the dWw / dbw
 *   partials, and dv[b, key, h, :] = sum_q P'd[b,h][q,key] dO[b, q, h, :] (P'd = dropout(proj_w(P)); element strides ob, on, oh; dv fp32 and /
 *   or dv16 bf16, either may be NULL).  Qf, Kf fp16 records (the forward's), dOf, Vf bf16 records (kind 0), dO16 = bf16 dO in the 16-wide layout
 *   (kind 1), c0 [B][Np][H] of spe_attn_merge_rows, Np >= 16 ceil(N / 16) + 64.
 * spe_talking_bwdq_pass2 (QUERY-major): dS = proj_l^T (P (dP - D)) as bf16 16 x 16 blocks (the dK contraction reads them), dWl / dbl partials,
 *   and dq[b, q, h, :] = scale * sum_key dS[b,h][q,key] k[b, key, h, :] accumulated in registers (element strides ob, on, oh; dq fp32 and / or
 *   dq16 bf16 with the same addressing, either may be NULL).  K16 = bf16 k in the 16-wide layout (kind 1).
 * keepbits: the dropout keep flags of spe_talking_flash_fwd, required when p_drop > 0.  Supported: H in {4, 8}, head dim <= 64 within the LDS
 * bound (H = 8: head dim <= 48); -2 otherwise. */
int spe_talking_bwdk_pass1(const void* Qf, const void* dOf, const void* dO16, const void* Kf, const void* Vf, const float* Wl, const float* Ww,
                           const float* bw, const float* c0, int Np, float* ws_d, float* ws_v, float* ws_w, float* Drows, float* dv, void* dv16,
                           long ob, long on, long oh, const void* keepbits, int B, int H, int N, int dh, int nwg, float p_drop, spe_stream_t stream);
int spe_talking_bwdq_plan(int B, int N, int nwg, int* steps_per_wg, int* nwg_used, int* nmajor);
int spe_talking_bwdq_pass2(const void* Qf, const void* dOf, const void* Kf, const void* Vf, const void* K16, const float* Wl, const float* Ww,
                           const float* c0, const float* Drows, int Np, float* ws_q, float* ws_w, void* dS, float* dq, void* dq16,
                           long ob, long on, long oh, float scale, const void* keepbits, int B, int H, int N, int dh, int nwg, float p_drop,
                           spe_stream_t stream);

/* ---- head-mean of the attention probabilities over heads and blocks (reference models/cait.py:384, 392 - a per-block clone of softmax(proj_l(
 * scale q k^T)) [B,H,N,N] - stacked and averaged by the woct0head backbone for cams_cls_patch, cait.py:993-994), accumulated without any
 * [B,H,N,N] tensor: M[b][q][k] += alpha * sum_g P_g[b][q][k] into a caller-owned fp32 M [B,N,N] (alpha = 1 / (depth * H): the mean).
 * spe_attn_pmean: P_g = exp2(sum_h Wl[g][h] S_h + c0[b][q][g]) recomputed from the fused forward's fp16 Qf / Kf records and the row constants c0
 *   [B][Np][H] of spe_attn_merge_rows (before proj_w and dropout).  Every 16 x 16 tile of M is read, added to and written by exactly one wave
 *   (no atomics: launches ordered on the stream give a deterministic sum).  H in {4,8}, head dim <= 64; -2 otherwise.
 * spe_attn_pmean_dense: the same from a materialised P [B,H,N,ld] (spe_talking_softmax_fwd's P; the fp32 path). */
int spe_attn_pmean(const void* Qf, const void* Kf, const float* Wl, const float* c0, int Np, float* M, float alpha, int B, int H, int N, int dh,
                   spe_stream_t stream);
int spe_attn_pmean_dense(const float* P, float* M, float alpha, int B, int H, int N, long ld, spe_stream_t stream);

/* ---- 3x3 convolutional class head (reference models/cait.py:971-974, 1142-1145, 1309-1312: Conv2d(C, K, 3, padding=1) over the normalised
 * patch tokens + AdaptiveAvgPool2d(1), and their autograd) as implicit GEMMs on the exact-fp32 matrix instruction, reading the tokens
 * x [B, h*w, C] channels-last as they are (no permute, no im2col).  W [K][C][3][3], bias [K].  Any B, h, w, K >= 1; C % 4 == 0; -2 otherwise.
 * spe_conv_head_fwd: map [B,K,h,w] = conv(x) + bias and logits [B,K] = its spatial mean, one launch (the mean crosses workgroups in fixed
 *   order: needs the reduction workspace, -4 without it).
 * spe_conv_head_plan: floats of the workspace spe_conv_head_bwd needs for the weight gradient.
 * spe_conv_head_bwd: with g = dmap + dlogits / (h w) (either may be NULL): dx [B, h*w, C], dW [K][C][3][3], db [K] (any may be NULL), all
 *   OVERWRITTEN.  dW / db are summed over positions in per-split partial rows of ws, added in split order (no atomics: bitwise reproducible). */
int spe_conv_head_fwd(const float* x, const float* W, const float* bias, float* map, float* logits, int B, int h, int w, int C, int K,
                      spe_stream_t stream);
int spe_conv_head_plan(int B, int h, int w, int C, int K, long* ws_floats);
int spe_conv_head_bwd(const float* x, const float* W, const float* dmap, const float* dlogits, float* dx, float* dW, float* db, float* ws,
                      long ws_floats, int B, int h, int w, int C, int K, spe_stream_t stream);

/* ---- streaming contractions of a blocked 16-bit score tensor T (dS of spe_talking_bwdq_pass2):
 *   trans = 0: out[b, q, h, :]   = alpha * sum_key T[b,h][q,key] x[b, key, h, :]   (`attn @ v`, cait.py:388; dQ)
 *   trans = 1: out[b, key, h, :] = alpha * sum_q   T[b,h][q,key] x[b, q, h, :]     (dV, dK of the same autograd)
 * X16 = spe_attn_pack16(x): bf16 [B,H,nt,ceil(dh/16)][64][4] = x[b, tile*16+4*(lane>>4)+i, h, dtile*16+(lane&15)]
 * (x element strides sb, sn, sh; 0 outside).  out element strides ob (batch), on (row), oh (head), unit d stride.
 * fmt: 0 = bf16 T x bf16 X16 (dQ, dK); 1 = fp16 T x fp16 X16, trans = 0 only (O = P'd V: pass alpha = 2^-8 for mode 1's scale);
 * 2 = fp16 T x bf16 X16, trans = 1 only (dV = P'd^T dO).
 * Head dim <= 64, returns -2 otherwise.  ws / counters (optional, both or neither): ws_floats floats of scratch and zero-
 * initialised 32-bit counters (at least B*H*2; left zero again by every launch) that let the launcher cut the groups of
 * output tiles beyond the last full round of resident workgroups into quarters of the contraction range, combined by the
 * last arriver in fixed order - without them every group is one workgroup.  One workspace serves all launches of a stream. */
int spe_attn_pack16(const float* x, long sb, long sn, long sh, int B, int N, int H, int dh, void* out, spe_stream_t stream);
/* njobs <= 6 packs of [B,Ns[i],H,dhs[i]] views in one launch: job i reads xs[i] (element strides strides[3i..3i+2] =
 * batch, row, head), multiplies by scales[i] and writes the spe_attn_pack (kinds[i] = 0), spe_attn_pack16 (1) or
 * full-32-steps-only (2: ceil(dh/32) steps of [lane][8], no tail step; spe_mha_*) layout to outs[i]; kinds[i] + 16: the same
 * layout with IEEE fp16 elements (saturating at +-65504) instead of bf16.  The pointer/stride tables are HOST arrays (copied
 * into the kernel arguments). */
int spe_attn_pack_multi(int njobs, const float* const* xs, const long* strides, const float* scales, const int* kinds,
                        void* const* outs, const int* Ns, const int* dhs, int B, int H, spe_stream_t stream);
int spe_attn_contract(const void* T, const void* X16, float* out, long ob, long on, long oh, int B, int H, int N, int dh,
                      int trans, int fmt, float alpha, float* ws, unsigned int* counters, long ws_floats, void* out16,
                      void* out16lo, spe_stream_t stream);

/* ---- out[c] (+)= sum_r in[r*ld + c] (bias gradients; autograd of nn.Linear bias; sums of split-K slabs).
 * accumulate = 1: added to what out holds (a zeroed buffer or a running sum); 0: out is overwritten (a weight gradient written
 * into its all-reduce bucket view needs no zeroing of the bucket beforehand). */
int spe_colsum(const float* in, float* out, long R, int C, long ld, int accumulate, spe_stream_t stream);

/* ---- LayerScale residual out = x + s_b*gamma*y (reference models/cait.py:413-416; s_b = the
 * per-sample DropPath keep scale or null).  bwd: dy = s_b*gamma*dout, dgamma += sum s_b*dout*y. */
int spe_layerscale_residual_fwd(const float* x, const float* y, const float* gamma, const float* sample_scale,
                                float* out, long R, int C, long rows_per_sample, spe_stream_t stream);
int spe_layerscale_residual_bwd(const float* dout, const float* y, const float* gamma, const float* sample_scale,
                                float* dy, float* dgamma, long R, int C, long rows_per_sample, spe_stream_t stream);
/* spe_layerscale_residual_bwd16: the same backward when the branch ends in a Linear on the bf16-copy GEMMs (proj / fc2 of
 * the backbone block, cait.py:390,412): dy = gamma * dout is emitted only as the bf16 operands of that Linear's backward
 * GEMMs - dy16 [R][C] and dy16T [C][ldt] (ldt = R rounded up to 64, padding zero) - with db[c] += sum_r dy (the Linear's
 * bias gradient, fp32 before rounding) and dgamma[c] += sum_r dout * y.  No per-sample scale (drop_path = 0).  y_f16 != 0: y holds
 * IEEE fp16 [R][C] (written by spe_gemm_bf16nt_ex with half_flags bit 0: y only ever enters this sum). */
int spe_layerscale_residual_bwd16(const float* dout, const void* y, int y_f16, const float* gamma, void* dy16, void* dy16T, long ldt,
                                  float* db, float* dgamma, long R, int C, spe_stream_t stream);
/* ... when the forward was out = x + s_b * gamma * dropout(y) (spe_gemm_bf16nt_exd): dy = s_b * keep * gamma * dout, dgamma += sum s_b * keep * dout * y. */
int spe_layerscale_residual_bwd16d(const float* dout, const void* y, int y_f16, const float* gamma, void* dy16, void* dy16T, long ldt,
                                   float* db, float* dgamma, long R, int C, float p_drop, uint64_t seed, uint64_t offset,
                                   const float* sample_scale, long rows_per_sample, spe_stream_t stream);

/* ---- activation backward: mode 1 ReLU (aux = forward output), mode 2 GELU (aux = pre-activation);
 * autograd of F.relu (transformer.py:32,287,424) and nn.GELU (timm Mlp). n % 4 == 0. */
int spe_act_bwd(const float* dy, const float* aux, float* dx, long n, int mode, spe_stream_t stream);

/* ---- norm(x + dropout(z)): the post-norm residual sites of the DETR encoder / decoder layers (reference
 * models/transformer.py:279-287, 384-386, 420-421, 426-427) in one pass each way.  fwd: sum = x + z*keepscale(row*C+c) (kept:
 * it is LayerNorm's input), y / mean / rstd as spe_layernorm_fwd.  bwd: ds = LayerNorm backward (gradient of x and of the sum),
 * dz = ds*keepscale with the same mask (not written when p == 0: the branch gradient is ds); dgamma / dbeta pre-zeroed; dy2 (optional): the
 * gradient of a second consumer of y - a post-norm layer's output feeds a Linear AND the next residual - added to dy while the row is loaded. */
int spe_layernorm_res_fwd(const float* x, const float* z, const float* gamma, const float* beta, float* sum, float* y,
                          float* mean, float* rstd, long R, int C, float eps, float p, uint64_t seed, uint64_t offset,
                          spe_stream_t stream);
int spe_layernorm_res_bwd(const float* dy, const float* dy2, const float* sum, const float* gamma, const float* mean, const float* rstd,
                          float* ds, float* dz, float* dgamma, float* dbeta, long R, int C, float p, uint64_t seed,
                          uint64_t offset, spe_stream_t stream);

/* ---- dropout y = x*keepscale (nn.Dropout at cait.py:387,391, transformer.py:266-288, timm Mlp);
 * the backward is the same call on dy. */
int spe_dropout(const float* x, float* y, long n, float p, uint64_t seed, uint64_t offset, spe_stream_t stream);

/* spe_rowops_plan: the kernel and grid that spe_colsum (launcher 0), spe_layerscale_residual_fwd (1), spe_layerscale_residual_bwd (2),
 * spe_layerscale_residual_bwd16 / _bwd16d (3), spe_act_bwd (4) and spe_dropout (5) choose for a shape.  Host only: no device, no stream,
 * nothing is launched; the launchers fill their launch from the same functions, so tests and tools can tell which branch a shape takes.
 * R, C: rows and columns (launchers 4 and 5: R = n, C ignored); ld: the leading dimension of spe_colsum's input, ldt of launcher 3, ignored
 * elsewhere; aligned: every pointer the launcher inspects is 16-B aligned (launchers 0, 2, 3).
 * v[4] = { kernel, grid.x, grid.y, members of the fixed-order sum across workgroups (csrc/det_reduce.h; 0: the kernel has none) };
 * kernel: 0 nothing is launched, 1 colsum_wide_kernel, 2 colsum_tall4_kernel, 3 colsum_kernel, 4 lsres_fwd_kernel,
 * 5 lsres_bwd_rows_kernel<16>, 6 lsres_bwd_kernel, 7 lsres_bwd16_kernel<2>, 8 lsres_bwd16_kernel<4>, 9 act_bwd_kernel, 10 dropout_kernel.
 * Returns the status the launcher would return for the shape (the rate / rows_per_sample refusals of _bwd16d and -4 aside); -2 for an
 * unknown launcher. */
int spe_rowops_plan(int launcher, long R, int C, long ld, int aligned, long* v);

/* ---- patch gather for the 16x16 stride-16 patch-embed conv (reference models/cait.py:518-528):
 * img[B,Cin,Hi,Wi] -> cols[B*(Hi/P)*(Wi/P), Cin*P*P] in conv-weight column order. */
int spe_patchify(const float* img, float* cols, int B, int Cin, int Hi, int Wi, int P, spe_stream_t stream);

/* ---- D[b][h][q] = sum_d x[b][q][h][d] y[b][q][h][d] for contiguous fp32 [B, L, H, dh] tensors (16-B aligned when dh % 4 == 0): the row term
 * rowsum(dO . O) of the softmax backward of the decoder's cross attention (autograd of reference models/attention.py:277-383). */
int spe_rowdot(const float* x, const float* y, float* D, int B, int L, int H, int dh, spe_stream_t stream);

/* ---- out = a + b[(i mod period)] (adds the interpolated pos-embed table, cait.py:623-624). */
int spe_add_rows(const float* a, const float* b, float* out, long n, long period, spe_stream_t stream);

/* ---- bicubic (A=-0.75, align_corners=false) resize of the learned position grid, token-major:
 * forward: src[gh*gw][C] -> dst[h*w][C]; backward=1: src = d(out)[h*w][C], dst = d(in)[gh*gw][C] PRE-ZEROED.
 * Reference models/cait.py:598-613 (F.interpolate(mode='bicubic')). */
int spe_bicubic(const float* src, float* dst, int gh, int gw, int h, int w, int C, int backward, spe_stream_t stream);

/* ---- Hungarian matcher cost (reference models/matcher.py:62-83 + util/box_ops.py:33-74):
 * logits[L,B,Q,Kc], boxes[L,B,Q,4] (cxcywh), targets concatenated over images with prefix
 * offsets toff[B+1].  cost[l] = packed concat over b of row-major [Q, M_b] blocks:
 * w_bbox*L1 + w_class*(pos_focal-neg_focal)[label] - w_giou*GIoU.  *err is OR-ed with 1 if a
 * degenerate box is seen (the reference's host assert, box_ops.py:64-65). */
int spe_matcher_cost(const float* logits, const float* boxes, const int* tgt_ids, const float* tgt_boxes,
                     const int* toff, int total_targets, float* cost, int* err, int L, int B, int Q, int Kc,
                     float w_class, float w_bbox, float w_giou, spe_stream_t stream);

/* ---- the assignment itself, on the device (reference models/matcher.py:83-86: scipy.optimize.linear_sum_assignment
 * per image on the host).  cost / toff as produced for spe_matcher_cost; every image needs M_b <= Q <= 1024 (-2
 * otherwise: fall back to the host).  Writes, for problem (l, b), M_b triples at offset l*total + toff[b] in ascending
 * query order: srow = (l*B+b)*Q + q, gidx = toff[b] + j (int64 each), lidx = l (int32).  fp64 potentials like SciPy.
 * err (device int, may be null; the flag word of spe_matcher_cost): bit 1 (value 2) is set when a problem has a row whose
 * remaining costs are all NaN / infinite (SciPy raises ValueError there); that problem gets the identity assignment. */
int spe_hungarian(const float* cost, const int* toff, long* srow, long* gidx, int* lidx, int* err, int L, int B, int Q,
                  spe_stream_t stream);
/* One-to-many target jitter (reference models/conditional_detr.py:409-431): out [M][ratio][4] - for every cxcywh box up to ratio - 1 of
 * its candidates scale[m][c][:] * box[m][:] (c < ncand, attempt order) whose IoU with the box exceeds 0.7, then the box itself for the
 * picks that found none and for the last row.  scale [M][ncand][4]: the uniform draws (the caller's generator), 16-B aligned. */
int spe_jitter_pick(const float* box, const float* scale, float* out, int M, int ncand, int ratio, spe_stream_t stream);

/* ---- weighted sigmoid focal loss (reference models/conditional_detr.py:468-494, 504-535):
 * logits[L*rows_per_l, Kc]; tclass[row] in [0,Kc] (Kc = no object); roww[row] row weight or
 * null.  loss[l] += sum (pre-zeroed by caller); grad = d(sum)/d(logit); argmax = top-1 class. */
int spe_focal_loss(const float* logits, const int* tclass, const float* roww, float* grad, float* loss,
                   int* argmax, int L, long rows_per_l, int Kc, float alpha, float gamma, spe_stream_t stream);

/* ---- matched-pair box losses (reference models/conditional_detr.py:300-319, 537-560):
 * pair i = (row srow[i] of pred_boxes[*,4], tbox[i], weight w[i] or null, layer lidx[i]).
 * sums[l][0] += w*L1, sums[l][1] += w*(1-GIoU) for l < L (pairs added in index order); g_l1/g_giou = d/d(pred cxcywh).
 * bwd scatter-adds c1[l]*g_l1 + c2[l]*g_giou into dpred rows. */
int spe_box_loss(const float* pred_boxes, const long* srow, const float* tbox, const float* w, const int* lidx,
                 float* sums, float* g_l1, float* g_giou, long n, int L, spe_stream_t stream);
int spe_box_loss_bwd(const long* srow, const int* lidx, const float* g_l1, const float* g_giou, const float* c1,
                     const float* c2, float* dpred, long n, spe_stream_t stream);

/* ---- memory side of the decoder's conditional cross attention for ALL layers (reference models/transformer.py:389-419):
 * spe_kv_frags turns the fp16 outputs of the two stacked projection GEMMs (spe_gemm_bf16nt with act bits 8 + 9) -
 *   ym16 [B*S][ldm]: column block 2l = ca_kcontent_proj_l(memory), 2l + 1 = ca_v_proj_l(memory);  yp16 [B*S][ldp]: block l =
 *   ca_kpos_proj_l(pos); d = H * dh columns per block -
 * into the operand fragments spe_mha_fwd / spe_mha_bwd consume, stacked over the layers ([L][B][H][ceil(S/16)] records):
 *   Kf  fp16, 32-wide steps of the 2 dh key dims [k_content | k_pos] of a head (spe_attn_pack_multi kind 2 + 16 layout)
 *   V16 fp16, 16-wide (kind 1 + 16);   K16 bf16, 16-wide (kind 1) and Vf bf16, 32-wide steps (kind 2): backward only, both or neither.
 * No fp32 key / value tensor, concatenation or per-layer pack.  dh % 8 == 0, dh <= 64, ldm / ldp % 8 == 0.
 * spe_kv_grad_scatter: dk [B,S,H,2 dh] / dv [B,S,H,dh] (fp32, spe_mha_bwd) of one layer -> bf16 column blocks 2l (content half of
 *   dk), 2l + 1 (dv) of dYm [B*S][ldm] and block l (pos half of dk) of dYp [B*S][ldp]: the stacked dY operands of the projection
 *   GEMMs' backward. */
int spe_kv_frags(const void* ym16, long ldm, const void* yp16, long ldp, void* Kf, void* V16, void* K16, void* Vf,
                 int L, int B, int S, int H, int dh, spe_stream_t stream);
int spe_kv_grad_scatter(const float* dk, const float* dv, void* dYm, long ldm, void* dYp, long ldp, int layer, int B, int S,
                        int H, int dh, spe_stream_t stream);
/* column sums of a bf16 matrix [R][ld] made of nblk (<= 32) column blocks of blkC columns, block i into its own fp32 vector outs[i]
 * (HOST array of device pointers): the bias gradients of the stacked projections, fixed summation order. */
int spe_colsum_bf16_blocks(const void* x, long ld, long R, int nblk, int blkC, float* const* outs, int accumulate, spe_stream_t stream);

/* ---- flash-style multi-head attention (reference models/attention.py:277-383; nn.MultiheadAttention core of the
 * encoder, models/transformer.py:275-277): softmax(scale q k^T + key_padding_mask), dropout, . v, forward and backward
 * without the [B,H,Lq,Lk] score tensor.  Operands are fragments from spe_attn_pack_multi: kind 2 (32-wide steps) of
 * q*scale*log2(e), k, v, dO -> Qf, Kf, Vf, dOf ; kind 1 (16-wide) of v, k, q*scale*log2(e), dO -> V16, K16, Q16, dO16.
 * Element formats: Qf, Kf and V16 FP16 (kinds + 16: the forward operands), Vf, dOf, K16, Q16, dO16 BF16.
 * q/k head dim <= 96, v head dim <= 64; mask [B,Lk] uint8 (1 = padded) or NULL; Philox dropout on element index
 * ((b*H+h)*Lq + q)*ld4 + key, ld4 = Lk rounded up to 4 (the stream spe_softmax_fwd draws from); the forward records the
 * keep flags in keepbits (B*H*ntq*ntk*4 64-bit words, needed when p_drop > 0) and the backward reads them.
 * spe_mha_plan: number of key chunks the forward / dQ kernels split the keys into (few query tiles -> many chunks).
 * spe_mha_fwd: Opart [B*H*ntq*nch][ceil(dv/16)][64][4] and ML [B*H*ntq*nch][16][2] floats of workspace ->
 *   O [B,Lq,H*dv], LSE [B,H,Lq] (log2 domain).  spe_mha_bwd: D [B,H,Lq] = rowsum(dO.O); with one key chunk dq [B,Lq,H,dk]
 *   is overwritten (no zero-initialising) and dq_ws is not read; with nch > 1 every chunk writes its own partial slab of
 *   dq_ws [nch][B*Lq*H*dk] (sum them with spe_colsum: no atomics, fixed order), dq is not touched, and dq_ws == NULL is
 *   refused with -2, nothing launched; dk [B,Lk,H,dk], dv [B,Lk,H,dv] are overwritten. */
int spe_mha_plan(int B, int H, int Lq, int Lk, int* nch);
int spe_mha_fwd(const void* Qf, const void* Kf, const void* V16, const void* mask, float* Opart, float* ML, float* O,
                float* LSE, void* keepbits, int B, int H, int Lq, int Lk, int dk, int dv, int nch, float p_drop,
                uint64_t seed, uint64_t offset, spe_stream_t stream);
int spe_mha_bwd(const void* Qf, const void* Kf, const void* Vf, const void* dOf, const void* K16, const void* Q16,
                const void* dO16, const void* mask, const float* LSE, const float* D, const void* keepbits, float* dq,
                float* dq_ws, float* dk, float* dv, int B, int H, int Lq, int Lk, int dk_dim, int dv_dim, int nch, float scale,
                float p_drop, spe_stream_t stream);

/* ---- sine position embedding of the padded feature map (reference models/position_encoding.py:37-57):
 * mask [B,h,w] uint8 (1 = padded), dim_t[npf] = temperature^(2*(k/2)/npf), out [B,h,w,2*npf] fp32 (row features first). */
int spe_pos_sine(const void* mask_u8, const float* dim_t, float* out, int B, int h, int w, int npf, float scale,
                 float eps, int normalize, spe_stream_t stream);

/* ---- learned position embedding of the patch grid (reference models/position_encoding.py:60-85: row_embed / col_embed =
 * nn.Embedding(50, npf), indexed by a cell's row / column; the padding mask is ignored, every image gets the same values).
 * spe_pos_learned_fwd: col, row [50][npf] -> out [B,h,w,2*npf] fp32, out[b][y][x][c] = col[x][c] for c < npf, row[y][c - npf] above
 *   (COLUMN features first - the opposite of spe_pos_sine - in the same buffer layout).
 * spe_pos_learned_bwd (the autograd of the two embedding lookups): g [B,h*w,2*npf] row-major fp32 ->
 *   d_col[x][c] = sum_b sum_y g[b][y][x][c], d_row[y][c] = sum_b sum_x g[b][y][x][npf + c].  All 50 rows of both [50][npf] gradients are
 *   OVERWRITTEN (rows >= w / >= h with zeros; the destination needs no zeroing); d_col or d_row NULL: that table is skipped.  One
 *   workgroup per output row adds its <= 50 B terms in an order fixed by the shape: no atomics, no reduction workspace, bitwise reproducible.
 * Any npf >= 1 (float4 lanes when npf % 4 == 0 and the pointers are 16-B aligned).  h or w outside 1 .. 50 (the reference's lookup raises
 * IndexError there), B < 1 or npf < 1: -2, nothing is launched. */
int spe_pos_learned_fwd(const float* col, const float* row, float* out, int B, int h, int w, int npf, spe_stream_t stream);
int spe_pos_learned_bwd(const float* g, float* d_col, float* d_row, int B, int h, int w, int npf, spe_stream_t stream);

/* ---- per-class greedy NMS (reference engine_loc.py:154-174: torchvision.ops.nms(boxes, scores, 0.5) per predicted
 * class, results concatenated in ascending class order).  boxes [nimg, nmax, 4] xyxy and labels [nimg, nmax] (int64)
 * ALREADY ordered by (label ascending, score descending) per image; counts[img] valid detections (NULL: nmax).
 * keep[img][i] = 1 iff detection i survives (suppress IoU > iou_threshold within a class).  nmax <= 4096. */
int spe_nms_sorted(const float* boxes, const long* labels, const int* counts, unsigned char* keep, int nimg, int nmax,
                   float iou_threshold, spe_stream_t stream);

/* ---- detection head (csrc/detect.hip): the detections of a batch in ONE launch - what PostProcess
 * (reference models/conditional_detr.py:592-623) followed by the per-class NMS above computes, without a host read.  One workgroup
 * per image, four phases, nothing goes to HBM between them:
 *   select   the top k of the N = Q * Kc logits of the image, ordered by logit descending, equal logits by flat index ascending.  The
 *            order is that of an order-preserving uint32 image of the float: -0.0 counts as +0.0, every NaN lies above +inf;
 *   decode   label = idx % Kc, query = idx / Kc; box = max(cxcywh -> xyxy, 0) * (w, h, w, h) in PostProcess's fp32 operations, one
 *            rounding each (no contraction); sizes[b] = (h, w);
 *   order    stable by label ascending: the order spe_nms_sorted expects;
 *   suppress (do_nms != 0) greedy per class, IoU > iou_threshold in spe_nms_sorted's arithmetic; survivors move to the front.
 * Outputs, every element written: out_logit [B][k] (the selected logits themselves, bit for bit), out_label [B][k] (int64), out_box
 * [B][k][4] xyxy absolute, out_query [B][k] (source query), out_count [B]; rows count .. k-1 hold logit -inf, label -1, box 0, query -1.
 * Integer LDS atomics only and every tie broken by index: bitwise reproducible.
 * Returns -3 when k < 1 or k > N (torch.topk raises), -2 when k > 1024 or N > 2^20; B <= 0: nothing to do. */
int spe_detect(const float* logits, const float* boxes, const float* sizes, int B, int Q, int Kc, int k, float iou_threshold,
               int do_nms, float* out_logit, long* out_label, float* out_box, int* out_query, int* out_count, spe_stream_t stream);

/* ---- CAM -> pseudo boxes (reference cams_deit.py:9-13 resize_cam, :61-96 get_multi_bboxes; engine.py:356-398).
 * spe_cam_prepare (device): M class maps cams[M][h][w] -> thresholded uint8 images out[M][rows][cols]: bilinear resize
 * (cv2.INTER_LINEAR convention), min-max normalisation, (x*255) truncated to uint8, THRESH_TOZERO at
 * int(cam_thr * max).  minmax: 2*M floats of workspace, contents need no initialisation.  Asynchronous.
 * spe_cam_contour_boxes (HOST function, host pointers): borders of the non-zero pixels of one image (Suzuki-Abe border
 * following, 8-connected, outer and hole borders = cv2.findContours RETR_TREE), polygon areas (cv2.contourArea) and the
 * boxes [x, y, x+w, y+h] (cv2.boundingRect) of every border with area >= area_ratio * largest, largest first;
 * [0,0,1,1] when there is none.  -5: more than max_boxes boxes. */
int spe_cam_prepare(const float* cams, int M, int h, int w, int rows, int cols, float cam_thr, float* minmax,
                    void* out, spe_stream_t stream);
int spe_cam_contour_boxes(const void* img, int rows, int cols, float area_ratio, int* boxes, int max_boxes, int* nboxes);
/* spe_cam_boxes_device (device, asynchronous, csrc/cambox_labels.hip): the same boxes in the same order for all M thresholded
 * images img[M][rows][cols] (uint8, what spe_cam_prepare writes) without leaving the device and without walking a border: two
 * connected-component labellings of the zero-padded image (foreground 8-connected, background 4-connected; union-find with
 * atomicMin, label = smallest pixel index), half-unit area counts per 2x2 window and boxes by integer atomics (bitwise
 * reproducible), every border's count folded into its ancestors in the border tree, the survivors collected per map and
 * ranked by one workgroup (formulation: csrc/cambox_index.h).
 * boxes[M][max_boxes][4] int32 [x, y, x+w, y+h], the first nboxes[m] rows of map m valid, the rest untouched; nboxes[m] = -5 when
 * map m has more than max_boxes survivors (none of its rows is written then), -6 if a label chain overran its bound (not reachable
 * by a valid image; the kernels give up instead of spinning).  1 <= max_boxes <= 2048.
 * workspace: caller-owned device memory, 16-B aligned, of at least the bytes spe_cam_boxes_device_workspace reports =
 * M * (7 * ((rows+2)*(cols+2) rounded up to 4) + 4 + 6 * 2048) * 4; contents need no initialisation.  -2: rows or cols < 1, more than 2^30
 * padded pixels, M > 65535, max_boxes out of range, workspace misaligned; -4: workspace NULL or too small.  M = 0: nothing launched.
 * spe_cam_boxes_device_workspace is a host function (bytes: host pointer). */
int spe_cam_boxes_device_workspace(int M, int rows, int cols, size_t* bytes);
int spe_cam_boxes_device(const void* img, int M, int rows, int cols, float area_ratio, void* workspace, size_t workspace_bytes,
                         int* boxes, int* nboxes, int max_boxes, spe_stream_t stream);

/* ---- training targets on the device (csrc/train_targets.hip): the step between the forward and the criterion of
 * the refine training loops (reference engine.py:356-398 and models/conditional_detr.py:641-677), without a host loop over boxes.
 * spe_cam_targets: packed = the result of spe_cam_boxes_device as it lies on the device, counts [M] then boxes [M][max_boxes][4] int32
 *   [x, y, x+w, y+h]; cls0 [M] (int32, device): the 0-based class of every map, the maps image-major with classes ascending.  Rows
 *   0 .. T-1 of boxes [cap][4] (fp32, 16-B aligned) and labels [cap] (int64) are the concatenation over the maps, in table order, of each
 *   map's first counts[m] boxes - single != 0: of its first box - as normalised cxcywh, label cls0[m] + 1; off [M + 1] (int32) is the
 *   first row of every map and off[M] = T.  A negative count is a status of spe_cam_boxes_device: it contributes no row and stays where
 *   it is for the caller to raise on.  Rows T .. cap-1 are not written.  The arithmetic is the host's, one rounding per operation:
 *   cx = float(x0 + x1) / 2.f / W, w = float(x1 - x0) / W, likewise y with H.  One workgroup: an exclusive scan over M in chunks with a
 *   carry, then one thread per row; asynchronous, nothing is read back.
 *   -2: M > 65535 or max_boxes > 2048 (the limits of spe_cam_boxes_device); -3: M < 0, max_boxes < 1, W or H < 1, a NULL or misaligned
 *   buffer, cap < M * (single ? 1 : max_boxes) - the counts are not known on the host, so the worst case must fit.  M = 0 writes off[0] = 0.
 * spe_refine_pick: prob [B][Q][Kc] (the sigmoid of the logits), pred_boxes [B][Q][4]; cls [U] (int32): per image its class ids, image b
 *   owning rows cls_off[b] .. cls_off[b+1] (int32 [B + 1]); both tables on the device, and once more on the HOST (cls_host, cls_off_host;
 *   NULL: unchecked) for the argument check.  For every row u of image b and class c: the best query of prob[b][.][c] by torch.max's rule
 *   - the largest value wins, equal values: the lowest query, a NaN beats every number and the first NaN wins - scores[u] = that value bit
 *   for bit, queries[u] (int32) = that query, boxes[u][4] = pred_boxes[b][query].  One wave per row, lanes stride over the queries, no
 *   atomics: bitwise reproducible.  Any Q >= 1; U = 0 and images without a class are valid (nothing launched for U = 0).
 *   -3: B < 0, Q < 1, Kc < 1, U < 0, a NULL buffer, host offsets that do not start at 0, descend or do not end at U, a host class id
 *   outside [0, Kc).  A device class id outside [0, Kc) that the host did not see reads nothing and leaves its row unwritten. */
int spe_cam_targets(const int* packed, const int* cls0, int M, int max_boxes, int single, int W, int H, int cap, float* boxes,
                    long* labels, int* off, spe_stream_t stream);
int spe_refine_pick(const float* prob, const float* pred_boxes, const int* cls, const int* cls_off, const int* cls_host,
                    const int* cls_off_host, int B, int Q, int Kc, int U, float* scores, int* queries, float* boxes, spe_stream_t stream);

/* ---- pseudo-label quality on the device (csrc/pseudo_quality.hip): CorLoc, precision, recall and mean IoU of the rows
 * the refine training loops feed their criteria, against the loader's ground-truth rows.  The reference reaches this view only through its
 * evaluator (engine_loc.py:204-220, pseudo_label_to_det_out); here it is ten int64 counters per class that stay on the device.
 * spe_pseudo_quality: pseudo rows of the batch concatenated, image b owning rows off[b] .. off[b+1] (int32 [B + 1], device): boxes [T][4]
 *   normalised cxcywh, labels [T] (int64), scores [T] or NULL; ground truth likewise with goff: gboxes [G][4], glabels [G].  Both offset
 *   vectors once more on the HOST (off_host, goff_host: required, the limits are checked on them before anything is launched).
 *   counters: int64 [10][C + 1], ACCUMULATED in place.  The IoU is box_iou on box_cxcywh_to_xyxy of both rows in fp32, one rounding per
 *   operation: corners cx -+ 0.5 * w, areas, max / min (a NaN on either side is the result), clamp(min=0), inter, (area1 + area2) - inter,
 *   the division.  Rules: a label outside [0, C) on either side is counted in column C of counters 4 / 7 and takes no further part.  Best
 *   IoU of a pseudo row: the maximum over the non-NaN IoUs with the same-label ground-truth rows of its image; without such a row it is an
 *   orphan.  Hit: best IoU > iou_thresh (strict).  A ground-truth row is covered when a same-label pseudo row of its image has
 *   IoU > iou_thresh with it.  Pair: an (image, class) with a ground-truth row.  Lead row of a pair: without scores the lowest pseudo row
 *   of the class, with scores the largest score by spe_refine_pick's rule (equal scores: the lowest row; the first NaN before everything).
 *   Counters per class: 0 pairs, 1 pairs whose lead row hits, 2 pairs with any hit, 3 pairs without a pseudo row, 4 pseudo rows, 5 rows
 *   that hit, 6 orphan rows, 7 ground-truth rows, 8 covered ground-truth rows, 9 the sum over the non-orphan rows of
 *   llrint(min(best, 1) * 2^20) for a finite positive best, else 0.
 *   One workgroup of 256 threads per image, the ground truth and both label vectors in LDS; integer atomics only: bitwise reproducible.
 *   Asynchronous, nothing is read back.  B = 0, or T = 0 and G = 0: status 0, nothing launched.
 *   -2: more than 1024 pseudo rows or 1024 ground-truth rows in one image.  -3: B, T or G < 0, C < 1, host offsets that are NULL, do not
 *   start at 0, descend or do not end at T / G, counters NULL, a NULL device buffer that has rows to hold. */
int spe_pseudo_quality(const float* boxes, const long* labels, const float* scores, const int* off, const float* gboxes,
                       const long* glabels, const int* goff, const int* off_host, const int* goff_host, int B, int T, int G, int C,
                       float iou_thresh, long* counters, spe_stream_t stream);

/* ---- proposal recall on the device (csrc/proposal_recall.hip): are the Q query boxes of a stage on the objects, or
 * is the pick among them wrong?  spe_pseudo_quality scores the one query per (image, class) that PostProcessRefine picks; this scores every
 * ground-truth row against ALL Q queries of its image.  The reference has no route to these numbers (its evaluator sees NMS survivors).
 * spe_proposal_recall: prob [B][Q][Kc] (the sigmoid of the logits) and boxes [B][Q][4] normalised cxcywh of one stage; ground truth of the
 *   batch concatenated, image b owning rows goff[b] .. goff[b+1] (int32 [B + 1], device; once more on the HOST as goff_host, required):
 *   gboxes [G][4] normalised cxcywh, glabels [G] (int64).  thr [T] and ks [K]: HOST tables, 1 <= T, K <= 8, thr finite and strictly
 *   ascending, ks >= 1 and strictly ascending (values above Q are allowed); they travel by value in the launch arguments.
 *   counters: int64 [2 + T + T * K][C + 1], ACCUMULATED in place: row 0 gts, 1 iou_q, 2 + t ceil[t], 2 + T + t * K + k hit[t][k].
 *   Rules, for a ground-truth row g of image b with label c:
 *   1. c outside [0, min(C, Kc)): gts[C] += 1 and nothing else.  Otherwise gts[c] += 1.
 *   2. iou[q] for all Q queries of image b: spe_pseudo_quality's IoU (box_iou on box_cxcywh_to_xyxy of both rows in fp32, one rounding per
 *      operation; csrc/box_iou_f32.h).
 *   3. best = the maximum over the non-NaN iou[q]; finite and > 0: iou_q[c] += llrint(min(best, 1) * 2^20).
 *   4. Per threshold t, S_t = { q : iou[q] > thr[t] } (strict; a NaN never covers).  Empty: nothing is counted for t.  Otherwise
 *      ceil[t][c] += 1; lead = the first element of S_t in class c's order of the image's queries by prob[b][q][c] - a NaN before every
 *      number, NaNs among themselves by lower q, larger values first, equal values (+0.0 == -0.0) by lower q: a total order whose first
 *      element is torch.max's and spe_refine_pick's pick; r = the number of queries of the image that precede lead in that order;
 *      hit[t][k][c] += 1 for every k with r < ks[k].
 *   One workgroup of 256 threads per image, the image's boxes as corners and areas in LDS, one wave per ground-truth row, O(T * Q) per
 *   row; integer atomics only: bitwise reproducible.  Asynchronous, nothing is read back.  B = 0 or G = 0: status 0, nothing launched.
 *   -2: Q > 1024 (the LDS staging).  -3: B or G < 0, Q, Kc or C < 1, T or K outside [1, 8], a table that is not strictly ascending, a
 *   threshold that is not finite, a cut-off < 1, host offsets that do not start at 0, descend or do not end at G, a NULL goff_host, thr,
 *   ks or counters, a NULL device buffer when something is launched.  All of it is checked before anything is launched. */
int spe_proposal_recall(const float* prob, const float* boxes, const float* gboxes, const long* glabels, const int* goff,
                        const int* goff_host, int B, int Q, int Kc, int G, int C, const float* thr, int T, const int* ks, int K,
                        long* counters, spe_stream_t stream);

/* ---- PASCAL VOC detection metrics (reference engine_loc.py:176-197, datasets/voc_eval.py, datasets/dis_eval.py; csrc/voc_eval.hip).
 * All arithmetic is fp64 in numpy's operation order, compiled without FMA contraction: with equal inputs the overlaps, and so every
 * threshold and tie decision, are bit-identical to the reference's.  Asynchronous; integer atomics only (bitwise reproducible).
 * spe_voc_match: greedy matching of one batch, one wave per (image, class).  Detections of all images concatenated, image i owning
 *   rows det_off[i] .. det_off[i+1] (int32, device), inside an image ALREADY ordered by (label ascending, score descending) - the order
 *   spe_nms_sorted's survivors have; det_boxes [nd][4] xyxy in 0-based pixels, det_scores [nd], det_labels [nd] (int64, class = label - 1).
 *   Ground truth likewise with gt_off [nimg+1]: gt_boxes [ng][4] fp64 in the annotation frame, gt_labels [ng] (int64), gt_difficult [ng].
 *   score_scale / coord_scale: the decimal round trip of the reference's result files - score -> rint(double(s) * score_scale) / score_scale,
 *   coordinate -> rint(double(x + 1.0f) * coord_scale) / coord_scale (the + 1 in fp32); 0: the raw double(s), double(x) + 1.0.
 *   A segment is visited in its incoming order; the overlap (+ 1. widths) is maximised over the ground truth of the class in the image,
 *   the FIRST maximum wins; ovmax > ovthresh (strict): non-difficult and unused -> tp and used, used -> fp, difficult -> neither;
 *   otherwise (also without ground truth, or with a NaN overlap) fp.
 *   flags [nd]: 0 ignored (difficult match, or a label outside 1 .. num_classes), 1 tp, 2 fp; scores_out [nd]: the (quantised) score
 *   as fp64; every one of the nd entries of both is written.  ADDED into the caller's int32 counters [num_classes]: npos (non-difficult
 *   ground truth), nimgs (images holding ground truth of the class), hits (CorLoc: the first detection of the segment overlaps ANY
 *   ground truth of the class, difficult ones included, by more than ovthresh).
 *   max_det / max_gt: the largest per-image counts in det_off / gt_off (the caller knows them from its shapes); more than 4096 / 1024:
 *   -2, nothing launched (an image whose offsets exceed them after all is skipped by the kernel).  nimg <= 0: nothing launched.
 * spe_voc_ap: one workgroup per class over flags sorted per class (class c owning seg_off[c] .. seg_off[c+1], int32, device; inside a
 *   class in curve order): tp / fp running counts, rec = tp / double(npos[c]), prec = tp / max(tp + fp, DBL_EPSILON), written to
 *   rec / prec (per detection; NULL: not stored); ap07[c]: the 11-point metric (voc_eval.py:32-40), ap_area[c]: the area under the
 *   precision envelope (voc_eval.py:41-56; terms added in a fixed order).  No detections: both 0; npos = 0: rec NaN, ap07 0, ap_area NaN. */
int spe_voc_match(const float* det_boxes, const float* det_scores, const long* det_labels, const int* det_off,
                  const double* gt_boxes, const long* gt_labels, const unsigned char* gt_difficult, const int* gt_off,
                  int nimg, int num_classes, int max_det, int max_gt, double ovthresh, double score_scale, double coord_scale,
                  unsigned char* flags, double* scores_out, int* npos, int* nimgs, int* hits, spe_stream_t stream);
int spe_voc_ap(const unsigned char* flags, const int* seg_off, const int* npos, int num_classes, double* ap07, double* ap_area,
               double* rec, double* prec, spe_stream_t stream);

/* ---- COCO detection metrics (reference engine.evaluate -> datasets/coco_eval.py: COCOeval for iouType 'bbox', useCats = 1;
 * csrc/coco_eval.hip).  fp64 in COCOeval's operation order, compiled without FMA contraction; asynchronous; integer atomics only.
 * The parameter arrays are the caller's (numpy's values, uploaded): iou_thrs [10], area_rng [4][2] (lo, hi), rec_thrs [num_rec]
 * ascending, max_dets [num_max_dets] (int32) - all in device memory.  A flag word holds, for one area range, the matched bits of the 10
 * thresholds in bits 0 .. 9 and the ignore bits in bits 10 .. 19.
 * spe_coco_match: greedy matching of one batch, one wave per (image, category).  Detections of all images concatenated, image i owning
 *   rows det_off[i] .. det_off[i+1] (int32), inside an image ALREADY ordered by (category index ascending, score descending, incoming):
 *   det_boxes [nd][4] xyxy fp32 in absolute pixels (w = x1 - x0 in fp32, then double; area = w * h in double), det_cats [nd] (int64
 *   category INDEX 0 .. num_cats-1; anything else belongs to no category).  Ground truth with gt_off [nimg+1]: gt_boxes [ng][4] xywh fp64,
 *   gt_cats [ng] (int64 index), gt_iscrowd [ng] bytes, gt_area [ng] fp64 (the annotation's field, not w * h).
 *   IoU of detection D and box G: w = min(D.x + D.w, G.x + G.w) - max(D.x, G.x), h likewise, 0 when either is <= 0, else
 *   (w * h) / (crowd ? D.area : D.w * D.h + G.w * G.h - w * h).  A box is ignored in area range a when it is crowd or its area is
 *   < lo or > hi.  Only the first `top` detections of an (image, category) are evaluated (maxDets' last entry).  Per (t, a) and detection:
 *   best = min(iou_thrs[t], 1 - 1e-10); the non-ignored boxes are walked in incoming order, then - only if none matched - the ignored
 *   ones; a box already matched at (t, a) is skipped unless it is crowd; iou < best skips, otherwise best = iou and the box is the
 *   match (so iou == threshold matches and the LAST of equal IoUs wins).  Matched: the ignore bit is the box's; unmatched: the
 *   detection is ignored when its area is outside the range.
 *   rank [nd] (int32): position inside the (image, category), or -1 for a detection that is not evaluated (past `top`, or no category);
 *   words [nd][4] (16-B aligned): the flag words (0 where rank = -1); every entry of both is written.  ADDED into npig [num_cats][4]
 *   (int32): the non-ignored boxes per category and area range.
 *   max_det / max_gt: the largest per-image counts; more than 4096 / 512, or top < 1: -2, nothing launched (an image whose offsets exceed
 *   them after all is skipped by the kernel).  nimg <= 0: nothing launched.
 * spe_coco_accumulate: one workgroup per (category k, area range a, max_dets entry m) over records sorted per category (category k
 *   owning seg_off[k] .. seg_off[k+1], int32; inside in curve order: score descending, image id ascending, rank); records with
 *   rank >= max_dets[m] take no part.  Per threshold t: tp / fp = running counts of the matched / unmatched records that are not ignored,
 *   rc = tp / npig[k][a], pr = tp / ((fp + tp) + 2^-52), pr made non-increasing from the end, and per rec_thrs[r] the first record with
 *   rc >= it gives precision [t][r][k][a][m] (the envelope there) and scores [t][r][k][a][m] (its score, widened), 0 past the end;
 *   recall [t][k][a][m] = the last rc, 0 without records.  npig[k][a] = 0: -1 everywhere.  Every element of the three is written.
 *   num_rec > 128 or < 1, num_max_dets < 1: -2. */
int spe_coco_match(const float* det_boxes, const long* det_cats, const int* det_off, const double* gt_boxes, const long* gt_cats,
                   const unsigned char* gt_iscrowd, const double* gt_area, const int* gt_off, const double* iou_thrs,
                   const double* area_rng, int nimg, int num_cats, int max_det, int max_gt, int top, int* rank, unsigned* words,
                   int* npig, spe_stream_t stream);
int spe_coco_accumulate(const unsigned* words, const int* rank, const float* det_scores, const int* seg_off, const int* npig,
                        const int* max_dets, const double* rec_thrs, int num_cats, int num_rec, int num_max_dets, double* precision,
                        double* recall, double* scores, spe_stream_t stream);

/* ---- multi-label classification AP (reference cams_deit.py:493-574, AveragePrecisionMeter.average_precision, the evaluator
 * engine.py and engine_loc.py import; csrc/cls_ap.hip).  Compiled without FMA contraction; asynchronous; no atomics at all.
 * Storage is class-major: class c owns scores[c * ld .. c * ld + n) (fp32) and targets[c * ld .. c * ld + n) (int8: 1 a positive, 0,
 * anything else - the caller reduces to -1 - a negative); nothing at or beyond column n of a row is read.  Per class the samples are
 * ranked: higher score first; scores that compare equal in fp32 (+0.0 and -0.0 included) by ascending sample index; a NaN score before
 * every number (where torch.sort(descending=True) puts it), NaNs among themselves by index.  A sample is counted unless difficult != 0
 * and its target is 0.  Walking the counted samples in rank order, every positive adds (double)pos_count / (double)total_count (both
 * counts include it) to an fp64 sum, in walk order, and ap[c] = sum / (double)npos[c]: with a tie-free column the number the
 * reference's Python loop returns, bit for bit.  npos[c] = 0: ap[c] = NaN (the reference raises ZeroDivisionError).
 * npos[c] / ncounted[c] (int32): the positives / the counted samples of the class.  n = 0: ap = NaN, both counts 0, workspace unused.
 * Two launches: one thread per (class, sample) counts the samples ranked at or before it by streaming the row through LDS - O(n^2)
 * comparisons per class - and stores a positive's term at slot pos_count - 1 of the class's workspace row; one workgroup per class adds
 * its npos[c] slots sequentially.  workspace: caller-owned device memory, 8-B aligned, n * C doubles (spe_cls_ap_workspace reports the
 * bytes; host function, bytes: host pointer); contents need no initialisation.  ap / npos / ncounted: [C], every element written.
 * -2, nothing launched: n < 0 or n > 2^24, C < 1 or C > 65535, ld < n; -4: workspace NULL with n > 0. */
int spe_cls_ap_workspace(int n, int C, size_t* bytes);
int spe_cls_ap(const float* scores, const signed char* targets, int n, int C, long ld, int difficult, double* workspace, double* ap,
               int* npos, int* ncounted, spe_stream_t stream);

/* ---- input transforms on the device (reference datasets/transforms.py + util/misc.collate_fn; csrc/img_resample.hip).
 * Pillow's Image.resize(..., BILINEAR) restated bit for bit: per axis, source length inS (after the crop) and output length outS,
 * in fp64 without FMA contraction: scale = inS / outS, fs = max(scale, 1), support = fs, ksize = (int)ceil(support) * 2 + 1; per
 * output xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), inS)
 * - xmin, w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fs|), normalised by their in-order sum, k[x] = (int)(0.5 + w[x] * 2^22);
 * out = clamp((2^21 + sum src[xmin + x] * k[x]) >> 22, 0, 255) in 32-bit integers.  Horizontal pass first, into uint8; the
 * vertical pass reads that uint8.  An unchanged axis gets the taps (2^22, 0): Pillow's copy.
 * Every launch serves n images, each through RS_DESC = 16 longs of a descriptor table that exists twice with equal content: desc_host
 * (HOST memory: validated, sizes the grids) and desc_dev (what the kernels read).  Fields: 0 src (device pointer, uint8 [srcH][srcW][3]),
 * 1 srcW, 2 srcH, 3 x0, 4 y0, 5 cw, 6 ch (the crop box in source pixels), 7 flip (view x -> x0 + (flip ? cw - 1 - x : x), y -> y0 + y:
 * crop and flip are an index map, never materialised), 8 ow, 9 oh (output size), 10 dst (device pointer, uint8 [oh][ow][3], for the
 * uint8 epilogue; else 0), and, written by spe_resample_plan: 11 byte offset into tmp, 12 / 13 int offsets of the x / y tables, 14 / 15
 * ksize of x / y.
 * Status: -2 empty box / output, a side above 32768, unplanned or inconsistent descriptors, an output larger than the batch;
 * -3 crop box outside the source; -5 ksize above the tap limit 65 (a 32x downscale; 4x needs 9).  A bad call launches nothing.
 * spe_resample_plan (host only): validates, fills fields 11 .. 15, totals[5] = bytes of tmp, ints of tables, max ow, max oh, max ch.
 * spe_resample_tables: xmin[outS], n[outS], k[outS][ksize] of both axes of every image, one launch.
 * spe_resample_h: view -> planar uint8 tmp [3][ch][ow rounded up to 4] per image.
 * spe_resample_v: out == NULL: tmp -> the uint8 HWC image dst of every descriptor (feeds another resize).  Else the final epilogue:
 *   out [n][3][Hmax][Wmax] fp32 = lut[c][byte] (lut: 3 x 256 fp32, ToTensor + Normalize as a table) inside [oh][ow] and 0 outside,
 *   mask [n][Hmax][Wmax] bytes = 0 inside and 1 outside; every element of both is written.  16-byte stores where the address is
 *   16-byte aligned, element stores at the unaligned head and tail of a row; Wmax is arbitrary. */
int spe_resample_plan(long* desc_host, int n, long* totals);
int spe_resample_tables(const long* desc_host, const long* desc_dev, int n, int* tables, spe_stream_t stream);
int spe_resample_h(const long* desc_host, const long* desc_dev, int n, const int* tables, unsigned char* tmp, spe_stream_t stream);
int spe_resample_v(const long* desc_host, const long* desc_dev, int n, const int* tables, const unsigned char* tmp, const float* lut,
                   float* out, unsigned char* mask, int Hmax, int Wmax, spe_stream_t stream);

/* ---- baseline JPEG decoding: the step in front of the transforms (the reference's datasets/voc.py and coco.py open every file
 * with PIL in __getitem__; csrc/jpeg_entropy.h + csrc/jpeg_decode.hip).  The result equals libjpeg-turbo's default decode - islow
 * IDCT, fancy upsampling, 16-bit fixed-point colour tables: what Pillow returns - bit for bit.
 * Host (plain C++, no HIP call, no global state: thread safe; data / info / coef / reason are HOST pointers):
 * spe_jpeg_probe: parses the markers up to the scan.  info [SPE_JPEG_INFO_INTS] ints: 0 width, 1 height, 2 components (1 or 3),
 *   3 / 4 luma sampling h / v, 5 restart interval, 6 / 7 MCUs across / down, 8.. / 11.. h / v per component, 14.. / 17.. blocks
 *   across / down per component (the grid padded to whole MCUs), 20.. blocks per component, 23 blocks in all, 24 the reason of a
 *   refusal, 25 offset of the entropy-coded data, 32.. the 8-bit quantisation table of every component, 64 values in natural order.
 * spe_jpeg_entropy: Huffman-decodes the one scan into coef: quantised int16 [blocks][64] in natural order, the components one
 *   after the other, each in raster order over its padded block grid; all blocks * 64 elements are written (zeros past an end of
 *   block).  coef_elems: elements the caller owns.  reason: NULL or one int.
 * Accepted: SOF0 with 8-bit samples and tables, one component or three with luma 1x1 / 2x1 / 2x2 over 1x1 chroma in one
 *   interleaved scan; DRI / RSTn; APPn and COM are skipped; EOI may be missing once every MCU is decoded.
 * Status: SPE_JPEG_UNSUPPORTED progressive, extended / lossless / arithmetic, 12-bit samples, 16-bit tables, two or four
 *   components, other sampling factors, several scans, Adobe APP14 with a transform other than 1, component ids R G B;
 *   SPE_JPEG_CORRUPT truncated data, a bad marker or segment length, a missing table, an undefined Huffman code, a run past
 *   coefficient 63, a wrong restart marker or unread bytes in front of one, a frame of more blocks than the data could hold at two
 *   bits a block (probe already: nobody allocates for a made-up size); -2 info NULL or coef too small.  No input makes either read or write outside
 *   [data, data + n) and the caller's buffers.
 * Device: spe_jpeg_reconstruct, two launches for n images, each through JD_DESC = 16 longs of a descriptor table that exists twice
 *   with equal content (desc_host validated, sizing the grids; desc_dev read by the kernels).  Fields: 0 W, 1 H, 2 components,
 *   3 / 4 luma sampling h / v, 5 / 6 MCUs across / down, 7 offset (int16 elements, a multiple of 8) of the image's record in coef,
 *   8 offset (bytes, a multiple of 16) of its planes in `planes`, 9 dst (device pointer, uint8 [H][W][3], any byte address).
 *   A record: 192 int16 (the three tables of spe_jpeg_probe) + blocks * 64 coefficients of spe_jpeg_entropy; planes: 64 bytes a block.
 *   Pass A: x = coef * q, jidctint.c's 8-point pass down the columns (descale 11) and along the rows (descale 18), the range limit
 *   t = (v + 128) & 1023, t < 256 ? t : t < 640 ? 255 : 0 -> uint8 planes.  Pass B: of a chroma plane ceil(W h / hmax) x
 *   ceil(H v / vmax) samples are real and neighbours clamp to them; 2x1: (3c + l + 1) >> 2, (3c + r + 2) >> 2; 2x2: s = 3c + the row
 *   above (even rows) / below (odd rows), then (3s + l + 8) >> 4, (3s + r + 7) >> 4; two or fewer real samples a row:
 *   replication instead; R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16), B = y + ((116130 cb + 32768)
 *   >> 16), clamped; one component: R = G = B = y.  Every byte of dst is written and nothing behind it: 4-byte stores where the
 *   address is aligned, byte stores at a row's head and tail.
 *   Status -2, nothing launched: n outside 1 .. 65535, a side outside 1 .. 32768, sampling or MCU counts that do not fit W and H,
 *   records or planes misaligned, overlapping, out of order or outside coef_elems / planes_bytes, dst 0, coef / planes not 16-B aligned. */
#define SPE_JPEG_UNSUPPORTED (-7)
#define SPE_JPEG_CORRUPT (-8)
#define SPE_JPEG_INFO_INTS 224
int spe_jpeg_probe(const unsigned char* data, long n, int* info);
int spe_jpeg_entropy(const unsigned char* data, long n, short* coef, long coef_elems, int* reason);
int spe_jpeg_reconstruct(const long* desc_host, const long* desc_dev, int n, const short* coef, long coef_elems,
                         unsigned char* planes, long planes_bytes, spe_stream_t stream);

/* ---- step ledger: the loss bookkeeping of a training step (reference engine.py:134-169, util/misc.py:34-93, 139-253;
 * csrc/step_ledger.hip, compiled without FMA contraction).  K loss values per step (1 <= K <= 256), E host scalars such as lr
 * (0 <= E <= 8), a ring of D = 64 steps, so a meter window is 1 .. 64.  Meters, in this order: K unscaled values, K scaled values
 * v * w (a key outside the mask keeps its slot, which is no meter of the reference and is never added to), `loss`, E extras:
 * M = 2K + 1 + E.  Single-workgroup launches, one thread (record) or one wave (summary) per meter, no atomics: bitwise reproducible.
 * state: caller-owned device memory, 8-B aligned, of at least the bytes spe_ledger_state_bytes reports (host function; bytes: host
 *   pointer); all-zero bytes are an empty ledger.  Layout: long steps, long first bad step + 1 (0: none), 2 longs reserved;
 *   double totals [M]; double extras ring [D][E]; float value ring [D][K]; float weight ring [D][K]; the newest mask [K], padded to 8.
 * spe_ledger_record: vals / weights [K] fp32, mask [K] bytes (non-zero: the key is in the weight dict; expected to stay the same
 *   through a run), extras_host [E] doubles in HOST memory (passed on by value).  scaled_k = v_k * w_k in fp32;
 *   total = ((0.0f + s_a) + s_b) + ... over the masked keys in index order by one lane - Python's sum() over fp32 tensors bit for
 *   bit - written to total [1]; v, w and the extras go to ring row step % D; (double)v_k, (double)scaled_k of masked keys,
 *   (double)total and the extras are added to the totals; steps += 1; a non-finite total records its step unless one is recorded
 *   already (sticky).  A non-finite value under an unmasked key records nothing; 0 * NaN under a masked key does.
 * spe_ledger_total_bwd: dvals[k] = mask[k] ? weights[k] * g[0] : 0 (g: the 0-dim upstream gradient).
 * spe_ledger_summary: out [M * 5 + 2] fp64: [M][5] = median, avg, global_avg, max, value of every meter over its last
 *   n = min(steps, window) steps, then steps and first bad step + 1 as doubles (one copy tells the host everything).  windows: [M] int32, the same table in host memory (validated) and in device memory (read by the kernel).
 *   ring_override: NULL, or a [D][K] fp32 ring that replaces the state's value ring (the rank-averaged one); weights, extras and
 *   totals always come from the state.  order: NULL, or [K] int32 - the key order in which `loss` is re-summed (the reference sums
 *   it in sorted key order once reduce_dict has rebuilt the dict).  Scaled values and `loss` are recomputed from the ring rows with
 *   the two expressions above.  median = float32 sorted[(n - 1) / 2] (ranks by counting, ties by position: torch.median's lower
 *   median), avg = float32(fp64 in-order sum / n), max = the largest, value = the newest, global_avg = totals / steps.  A NaN in
 *   the window makes median and max NaN.  steps = 0: every field NaN.
 * Status, before any launch: -2 K or E out of range, a window outside 1 .. 64, a NULL pointer other than the state, ring_override
 *   and order (extras_host may be NULL when E = 0); -4 state NULL, misaligned or smaller
 *   than spe_ledger_state_bytes.  A refused call writes nothing. */
int spe_ledger_state_bytes(int K, int E, size_t* bytes);
int spe_ledger_record(const float* vals, const float* weights, const unsigned char* mask, const double* extras_host, int K, int E,
                      void* state, size_t state_bytes, float* total, spe_stream_t stream);
int spe_ledger_total_bwd(const float* g, const float* weights, const unsigned char* mask, int K, float* dvals, spe_stream_t stream);
int spe_ledger_summary(void* state, size_t state_bytes, int K, int E, const int* windows_host, const int* windows_dev,
                       const float* ring_override, const int* order, double* out, spe_stream_t stream);

/* ---- optimiser step on flat buffers (reference engine.py:161-165: clip_grad_norm_(params, 0.1) + AdamW.step(),
 * parameter groups of main.py:177-191).  spe_sqnorm_partials: partials[b] = sum g^2 over the b-th of nblocks chunks.
 * spe_adamw_flat: clip = min(1, max_norm / (sqrt(sum partials) + 1e-6)) (max_norm <= 0: no clipping), g *= clip,
 * then torch.optim.AdamW's update with bias corrections bias_c1 = 1 - beta1^t, bias_c2 = 1 - beta2^t; element i uses
 * (lr, weight decay) of the segment s with seg_end[s-1] <= i < seg_end[s] (nseg <= 64).  write_grad != 0 stores the
 * clipped gradient back (what clip_grad_norm_ leaves in .grad).  Buffers 16-B aligned.  grad_scale: g is first multiplied
 * by it (1/world after a SUM all-reduce: DistributedDataParallel's gradient averaging, reference main.py:172, folded into
 * this launch); the clip norm is that of the scaled gradient. */
int spe_sqnorm_partials(const float* g, long n, float* partials, int nblocks, spe_stream_t stream);
int spe_adamw_flat(float* p, float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr,
                   const float* seg_wd, int nseg, float beta1, float beta2, float eps, float bias_c1, float bias_c2,
                   const float* partials, int npartials, float max_norm, int write_grad, float grad_scale,
                   spe_stream_t stream);

/* ---- the same step, skipped on the device when the reduced gradient is not finite (reference engine.py:147-159 exits before
 * optimizer.step() on a non-finite loss; here the decision sits where the norm already is, no host read).  Per optimizer step:
 * spe_sqnorm_partials for every bucket, ONE spe_adamw_gate, then spe_adamw_flat_guarded per bucket.
 * The guard block: SPE_ADAMW_GUARD_WORDS 4-byte words, 16-B aligned, zeroed by the caller before the first step.
 *   int32 [0] applied steps   [1] skipped steps   [2] 1-based attempt index (applied + skipped) of the first skipped step, 0: none
 *         [3] apply: this step's decision (1 / 0)
 *   fp32  [4] clip * grad_scale of this step (0 when skipped)   [5] 1 - beta1^t   [6] sqrt(1 - beta2^t)   [7] the gradient norm
 *         grad_scale * sqrt(sum partials) (inf / NaN when skipped)   [8] applied steps as a float (torch's `step` entry)
 *   words 9 .. 15 are reserved and never written.
 * spe_adamw_gate (one workgroup): sums partials[0 .. npartials) - the partials of ALL buckets - with the reduction spe_adamw_flat
 * uses, so clip = min(1, max_norm / (norm + 1e-6)) has the bits of the unguarded path (max_norm <= 0: no clipping; the sum is
 * taken all the same).  apply = isfinite(sum): a NaN or an infinity anywhere in the buckets skips the step, and so does a squared
 * norm that overflows fp32 (an element beyond ~1.8e19 is enough).  t is the APPLIED count including this step - a skipped step
 * does not shift the bias corrections of later ones; beta^t is taken in fp64 and rounded to fp32 once.  One lane writes the block
 * with ordinary stores.  -2: guard NULL or misaligned, partials NULL, npartials < 1.
 * spe_adamw_flat_guarded: spe_adamw_flat with the block in place of bias_c1, bias_c2, partials, max_norm and grad_scale.  Every
 * workgroup reads the record; with apply == 0 it returns before its first store (p, g, m, v keep their bits, whatever
 * write_grad says), otherwise the per-element arithmetic is spe_adamw_flat's (one kernel body).  Status as spe_adamw_flat: -2
 * for misaligned buffers (the block included) or nseg outside 1..64, 0 and no launch for n <= 0. */
#define SPE_ADAMW_GUARD_WORDS 16
int spe_adamw_gate(void* guard, const float* partials, int npartials, float max_norm, float grad_scale, double beta1,
                   double beta2, spe_stream_t stream);
int spe_adamw_flat_guarded(float* p, float* g, float* m, float* v, long n, const long* seg_end, const float* seg_lr,
                           const float* seg_wd, int nseg, float beta1, float beta2, float eps, const void* guard,
                           int write_grad, spe_stream_t stream);

/* ---- gradient accumulation beside the flat buckets (reference engine.py:161-165 together with main.py:170-172: ONE
 * optimizer step over world x batch images; on fewer GPUs the missing ranks become micro-steps, spe_amd/dp.py accum_steps).
 * dst[i] = a[i] + b[i]; b == NULL: the bit copy dst[i] = a[i] (-0.0 and NaN payloads survive).  dst may alias a or b.
 * Every pointer 16-B aligned (-2 otherwise, nothing written); n <= 0: nothing launched.  No atomics, no cross-lane sums:
 * bitwise deterministic. */
int spe_accum_flat(float* dst, const float* a, const float* b, long n, spe_stream_t stream);

/* ---- weight EMA inside the update launch (no reference site: the reference's evaluate / evaluate_refinements, engine.py:448 and
 * :617, read the last iterate; the DETR family's usual remedy for a noisy last iterate, kept here as one more fp32 stream of the launch that exists anyway).
 * spe_adamw_flat_ema: spe_adamw_flat (guard == NULL) or spe_adamw_flat_guarded (guard != NULL: the block of spe_adamw_gate; bias_c1,
 * bias_c2, partials, npartials, max_norm, grad_scale and t are then ignored) with one more flat buffer e of the same layout:
 *     e'[i] = e[i] + w * (p'[i] - e[i])        three fp32 operations, each rounded (no FMA), p' the parameter just computed
 *     w = (float)(1 - d),  d = warmup ? min(decay, (1 + t) / (10 + t)) : decay    in fp64, rounded once
 * t: the 1-based count of applied steps including this one - the argument (unguarded) or word [8] of the guard block (guarded).  p,
 * g, m and v get the bits the entry without the EMA leaves.  Padding elements are averaged like the rest.  A guarded launch that
 * reads apply == 0 writes nothing: e keeps its bits and the warm-up does not advance.  Status as the two entries above; -2 also for
 * e NULL or not 16-B aligned and for decay outside [0, 1) (NaN included).  One kernel body and one launch helper serve all three entries.
 * spe_swap_flat: exchanges the bits of a[0 .. n) and b[0 .. n) (loads and stores only: NaN payloads and -0.0 survive); the grid of
 * spe_accum_flat.  -2: a pointer NULL or not 16-B aligned, a == b; n <= 0: nothing launched. */
int spe_adamw_flat_ema(float* p, float* g, float* m, float* v, float* e, long n, const long* seg_end, const float* seg_lr,
                       const float* seg_wd, int nseg, float beta1, float beta2, float eps, float bias_c1, float bias_c2,
                       const float* partials, int npartials, float max_norm, int write_grad, float grad_scale,
                       const void* guard, double decay, int warmup, long t, spe_stream_t stream);
int spe_swap_flat(float* a, float* b, long n, spe_stream_t stream);

/* ---- per-parameter gradient report on the flat buckets (no reference site: the reference exits on a non-finite loss, engine.py:147-159,
 * and logs no per-layer norms).  The guarded step can only count its skips; this entry says which parameter carried the NaN, the
 * infinity or the finite element whose square overflows, and gives the gradient / weight norms of every parameter.
 * g, p: the flat gradient and parameter buffers of one bucket, n elements each, 16-B aligned; p may be NULL.  par_beg / par_len: device
 * tables of npar entries, parameter i is g[par_beg[i] .. par_beg[i] + par_len[i]) (and the same range of p); what lies between the
 * parameters is never read.  The table contents are TRUSTED, as seg_end of spe_adamw_flat is: ranges inside [0, n), par_len < 2^31.
 * A parameter may start anywhere (one that does not start on a 16-B boundary is read with 4-B loads: same values, same record).
 * out: npar records of SPE_GRAD_REPORT_WORDS 4-byte words, 16-B aligned:
 *   fp32  [0] sum of (grad_scale * g)^2 over the finite elements of g   [1] max |grad_scale * g| over them (0 if there are none)
 *         [2] sum of p^2   [3] max |p| (a NaN in p is ignored by the maximum and makes [2] NaN)      - both 0 with p == NULL
 *   int32 [4] NaN elements of g   [5] +-inf elements of g   [6] index within the parameter (row-major) of the first non-finite element
 *         of g, -1 if none   [7] the attempt index at the time of writing: guard words [0] + [1]; 0 with guard == NULL
 * Arithmetic: fp32 throughout, every operation rounded on its own (no FMA, no fp64): s = grad_scale * g, q = s * s, then additions.  A
 * finite element beyond ~1.8e19 therefore shows in [0] as inf, exactly as it overflows the guard's norm.  A non-finite element of g is
 * counted and then taken as +0.0: the record is, bit for bit, that of the same tensor with those elements replaced by +0.0.
 * grad_scale is finite.
 * Order of the two sums of a parameter of L elements (x_j = q of element j, +0.0 for j >= L).  The parameter is cut into chunks of
 * 16384 elements counted from its own first element; chunk c (elements 16384 c ...) is summed by one workgroup of T = 256 lanes:
 *   1. vector v = 0, 1, ... of the chunk holds its elements 4v .. 4v + 3 and is reduced to   y_v = (x_4v + x_4v+1) + (x_4v+2 + x_4v+3);
 *   2. lane t adds its vectors in ascending order:   a_t = ((0 + y_t) + y_(t+T)) + y_(t+2T) + ...   (pass k covers the chunk's
 *      elements 1024 k .. 1024 k + 1023; 16 passes at most);
 *   3. inside each wave of 64 consecutive lanes, six xor-butterfly steps   a_t <- a_t + a_(t xor o),  o = 32, 16, 8, 4, 2, 1;
 *      every lane of the wave ends with the same bits;
 *   4. the 4 wave sums are added in ascending wave order starting from 0:   P_c = (((0 + w_0) + w_1) + w_2) + w_3;
 * and a second launch adds the chunk sums in ascending chunk order starting from 0:   ((0 + P_0) + P_1) + ...
 * The record is thus a pure function of the parameter's values and length: it does not depend on par_beg, npar, n or the other
 * parameters.  Maxima, counts and the first index are exact and order-free.  No atomics; one lane stores a record as two 16-B words.
 * The chunk records pass through the reduction workspace (spe_set_reduce_workspace; 32 bytes for each of n / 16384 + npar slots) from
 * the first launch to the second: launches must be stream-ordered, as for every user of that workspace.
 * when: gating on the guard block of spe_adamw_gate - 0: always write (guard may be NULL); 1: write only if guard [3] (apply) is 0,
 * i.e. this step is skipped; 2: only if apply == 0 and guard [1] (skipped) is 1, the first skipped step.  A workgroup that finds the
 * condition false returns after reading the guard words and nothing else: out keeps every bit.
 * -2: g or out NULL or not 16-B aligned, p or guard not 16-B aligned, a table NULL, npar < 1, when outside 0..2, when != 0 with
 * guard NULL.  -4: no reduction workspace registered, or too small for the slots.  n <= 0: status 0, nothing launched. */
#define SPE_GRAD_REPORT_WORDS 8
int spe_grad_report(const float* g, const float* p, long n, const long* par_beg, const long* par_len, int npar,
                    float grad_scale, const void* guard, int when, void* out, spe_stream_t stream);

/* ---- diagnostic (never launched by the product): keep nwg workgroups resident for `micros` microseconds, streaming copies
 * through buf (buf_floats floats, 16-B aligned; NULL: idle spinning) - the one-GPU proxy for the CU / HBM share of an RCCL ring
 * running beside the backward (reference main.py:172: DistributedDataParallel overlaps its all-reduce with the backward);
 * tools/dp_proxy.py measures the slowdown of the step under it. */
int spe_occupy(int nwg, long micros, float* buf, long buf_floats, spe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPE_HIP_H */
