/*
 * gptq_mi355x.h -- C ABI of libgptq_mi355x.so: the MI355X (gfx950) native hot path behind
 * GPTQ-for-LLaMa's `quant.QuantLinear` operator family.
 *
 * Every entry point is what a binding of the reference's operator interface for this path
 * would call; the reference symbol each one stands in for is cited as
 * `file:line` into qwopqwop200/GPTQ-for-LLaMa (triton branch).  There are no torch types in
 * the signatures: plain device pointers, sizes, a HIP stream.  The caller owns every buffer;
 * the library allocates nothing, never synchronises and never throws -- all launches go to
 * `stream` and are hipGraph-capturable.
 *
 * Buffer conventions (identical to the reference checkpoint format, quant_linear.py:316-321):
 *   x        fp16 [M, K]      row stride ldx (elements), last dim contiguous
 *   qweight  int32 [K/32*bits, N]  row-major; bits in {2,4,8}: word r holds k = r*f .. r*f+f-1
 *            (f = 32/bits) of one column, field j at bit bits*j (quant_linear.py:103,109,127).
 *            bits == 3 (EXTENSION, the reference raises NotImplementedError,
 *            quant_linear.py:308-309): 32 consecutive k of a column are a dense little-endian
 *            96-bit stream over 3 consecutive rows.
 *   qzeros   int32 [G, N/32*bits]   same packing along n; stored value is zero-1 and the
 *            kernel adds 1 WITHOUT re-masking (quant_linear.py:120-121)
 *   scales   fp16 [G, N]
 *   g_idx    int32 [K] group of each k, or NULL meaning the trivial map k / groupsize
 *   bias     fp16 [N] or NULL; added after the fp16 rounding of the product
 *            (separate torch add in the reference, quant_linear.py:376)
 *   y        fp16 [M, N]      row stride ldy
 *   G = ceil(K / groupsize); groupsize == K for the reference's "-1".
 *
 * Return value: 0 on success; negative = GPTQ_E_* (bad argument, nothing launched);
 * positive = hipError_t from a launch.
 */
#ifndef GPTQ_MI355X_H
#define GPTQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *gptq_stream_t; /* hipStream_t */

enum {
    GPTQ_OK = 0,
    GPTQ_E_BITS = -1,      /* bits not in {2,3,4,8}             (quant_linear.py:308-309)  */
    GPTQ_E_SHAPE = -2,     /* K or N not a multiple of 32, M < 0, groupsize <= 0            */
    GPTQ_E_ALIGN = -3,     /* pointer / leading dimension alignment                          */
    GPTQ_E_NULL = -4,      /* required pointer is NULL                                       */
    GPTQ_E_WORKSPACE = -5, /* workspace too small for the requested variant                  */
    GPTQ_E_VARIANT = -6,   /* unknown / inapplicable kernel variant                          */
    GPTQ_E_NORM_WIDTH = -7,/* RMSNorm row wider than 64 KiB (triton_norm.py:59-60)           */
    GPTQ_E_LIBRARY = -8    /* prefill route: hipBLASLt not loadable, or it refused the product */
};

/* gptq_query(what) */
enum {
    GPTQ_Q_ABI_VERSION = 0,
    GPTQ_Q_GEMV_MAX_M = 1,        /* largest M of the rowwave GEMV family (4-bit: M <= 4 rows share one launch) */
    GPTQ_Q_SKINNY_MAX_M = 2,      /* largest M served by the weight-streaming MFMA kernel    */
    GPTQ_Q_WORKSPACE_BYTES = 3,   /* bytes of zero-initialised workspace split-K needs       */
    GPTQ_Q_NUM_GEMV_VARIANTS = 4,
    GPTQ_Q_STRIPE_MM_WORKSPACE_BYTES = 5   /* bytes of the (separate, scratch) workspace of gptq_stripe_matmul_f16 */
};

int gptq_query(int what);
const char *gptq_strerror(int code);

/* Dispatch override used by the tests and the sweeps: variant < 0 restores the built-in choice.
 * For the rowwave GEMV variant v selects U = 8 >> v packed rows in flight per wave (v in 0..2; 3-bit:
 * 2 >> v 32-k blocks, v in 0..1) and is refused (GPTQ_E_VARIANT) when U does not divide the group;
 * for the weight-streaming MFMA kernel the values 2, 4, 8 select the waves per workgroup.
 * gptq_set_split_k forces the number of K slices (>= 1).  Both return the previous value. */
int gptq_set_gemv_variant(int variant);
int gptq_set_split_k(int split_k);
/* Prefill GEMM kernel selection (tests / A-B measurements): 2 = ping-pong kernel (default), 3 = all-LDS-DMA
 * kernel with packed B in LDS (4-bit, groupsize % 64 == 0; measured 2-4 % slower).  Returns the previous value. */
int gptq_set_gemm_kernel(int version);
/* Prefill route behind gptq_prefill_matmul_f16 / _fused_mlp_f16 / _transpose_matmul248_f16 (tests / A-B measurements):
 * 1 (default) = the hand-written LDS-DMA + MFMA tile GEMM of csrc/gemm8.hip on the dequantised weight wherever it can run
 * (K % 128 == 0: every LLaMA shape) -- since round 4 the default route never reaches hipBLASLt for such shapes; 2 = the same (kept for
 * callers of earlier rounds); 0 = hipBLASLt only (the reported ceiling).  Returns the previous value. */
int gptq_set_prefill_route(int route);
/* Rows per pass of the 16-row MFMA tiles on the stripe16 image (gptq_stripe_matmul_f16, the 5..128-row route of gptq_layer_forward):
 * 128 (default: 65..128 rows in ONE pass over the weights) or 64 (round 2's schedule; A-B runs).  Returns the previous value. */
int gptq_set_stripe_mm_pass_rows(int rows);
/* Batches of 129 .. `rows` rows of a layer with a stripe16 image run the fused-dequantise tile GEMM on the image (csrc/stripe_mm.inc,
 * stripe_gemm_kernel: weights stay packed, no per-call dequantise pass) instead of the dense route; 0 = never (tests / A-B runs).
 * Round 5: gptq_layer_forward keeps a trivial-g_idx layer on the image only while its 128 x 128 tiles fit the chip at once
 * (ceil(M / 128) * N * nsets / 128 <= 512) or M <= 640 (gate | up pair: 1152); above, dequantise + the tile GEMM is the faster own kernel
 * (gptq_layer_route_for_shape says which; gptq_stripe_matmul_f16 itself serves every M up to `rows`).  Returns the previous value. */
int gptq_set_stripe_gemm_max_rows(int rows);
/* which engine a dense product of this shape takes under the current switch: 1 = tile GEMM, 0 = hipBLASLt (host logic only;
 * nsets = 2: gate/up pair; trans = 1: the backward product) */
int gptq_prefill_route_for(int M, int K, int N, int nsets, int trans);
/* test hooks: make every library call answer GPTQ_E_LIBRARY as if hipBLASLt were not installed (returns the previous setting);
 * number of hipBLASLt plans currently cached (bounded LRU of 64) */
int gptq_set_library_enabled(int on);
/* MFMA shape of the tile GEMM (tests / A-B runs): 16 = v_mfma_f32_16x16x32_f16, 32 = v_mfma_f32_32x32x16_f16; returns the previous value */
int gptq_set_gemm8_mfma(int shape);
/* Rows of the tile GEMM's workgroup tile: 0 = chosen per launch (the tile whose rounds of 256 workgroups cost less), 192, 256.  Returns the
 * previous value, GPTQ_E_VARIANT for anything else.  Results do not depend on it (same K order per accumulator).  Test / A-B hook. */
int gptq_set_gemm8_tile(int rows);
int gptq_prefill_plan_count(void);
/* Development aid: when non-NULL, the decode kernels write per-wave s_memtime checkpoints
 * ([block][wave][8] uint64) into this device buffer.  Returns the previous pointer. */
void *gptq_set_debug_buffer(void *device_buffer);
/* Test support: one launch that overwrites all 160 KB of LDS on every CU with (pattern ^ word index) -- the soak test interleaves it with the decode
 * launches: no kernel of this library may read LDS it has not written (tests/test_gpu_soak.py). */
int gptq_debug_dirty_lds(uint32_t pattern, gptq_stream_t stream);
/* debug hook: device uint32 that every stripe16 decode launch (M = 1) increments (one relaxed device-scope add) when it starts; NULL
 * (default) = no tick.  Used by tools/warmlab.hip to pace a run-ahead prefetcher on a second stream (measured, loses: DESIGN 3.6). */
int gptq_set_progress_counter(void *device_u32);

/*
 * y = x . deq(B) (+ bias)  -- reference matmul248() + matmul_248_kernel + the bias add in
 * QuantLinear.forward (quant/quant_linear.py:263-269, :72-137, :373-377).
 * Chooses the rowwave GEMV (M = 1; 2 <= M <= 4 at 4 bits: all rows in one launch), the weight-streaming MFMA
 * kernel (M <= 64) or the tiled MFMA GEMM (prefill).  workspace: >= gptq_query(GPTQ_Q_WORKSPACE_BYTES) bytes, zero on first
 * use, one per device and per stream of execution (its first 516 KiB -- combine words and arrival tickets --
 * are restored to zero by every launch, the rest is scratch); may be NULL, which disables the K split.
 */
int gptq_matmul248_f16(const void *x, int64_t ldx, const int32_t *qweight, const void *scales,
                       const int32_t *qzeros, const int32_t *g_idx, const void *bias, void *y,
                       int64_t ldy, int M, int K, int N, int bits, int groupsize, void *workspace,
                       size_t workspace_bytes, gptq_stream_t stream);

/* Round 6: the fp32 partial product of a ROW SHARD of a layer with ANY g_idx -- what a tensor-parallel rank computes for o_proj / down_proj of an
 * act-order checkpoint (the reference has no tensor parallelism: llama.py:328-382 places whole layers; north_star: K-shards, fp32 partials, ONE
 * all-reduce and ONE fp16 rounding per linear).  The shard's k range is fixed by the rank's heads / gate-up columns, so its rows point into all
 * groups of the layer: qweight = the shard's K / 32 * bits packed rows, scales [n_groups][N] / qzeros [n_groups][N / 32 * bits] = the WHOLE
 * layer's tables, g_idx [K] = the group of each of the shard's rows (required).  y32[M][ldy] = x[M][K] . dequant(W shard), sums left in fp32
 * (weights dequantised as matmul_248_kernel does, quant_linear.py:128; fp32 accumulate).  Replaces the fp16-output generic launch that cost one
 * extra rounding per rank. */
int gptq_matmul248_partial_f32(const void *x, int64_t ldx, const int32_t *qweight, const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                               float *y32, int64_t ldy, int M, int K, int N, int bits, int n_groups, gptq_stream_t stream);

/* Same contract, forcing one kernel family (tests and benchmarks). */
int gptq_gemv_f16(const void *x, int64_t ldx, const int32_t *qweight, const void *scales,
                  const int32_t *qzeros, const int32_t *g_idx, const void *bias, void *y,
                  int64_t ldy, int M, int K, int N, int bits, int groupsize, void *workspace,
                  size_t workspace_bytes, gptq_stream_t stream);
int gptq_skinny_f16(const void *x, int64_t ldx, const int32_t *qweight, const void *scales,
                    const int32_t *qzeros, const int32_t *g_idx, const void *bias, void *y,
                    int64_t ldy, int M, int K, int N, int bits, int groupsize, void *workspace,
                    size_t workspace_bytes, gptq_stream_t stream);
int gptq_gemm_f16(const void *x, int64_t ldx, const int32_t *qweight, const void *scales,
                  const int32_t *qzeros, const int32_t *g_idx, const void *bias, void *y,
                  int64_t ldy, int M, int K, int N, int bits, int groupsize, gptq_stream_t stream);

/*
 * c = silu(x . deq(B_gate)) * (x . deq(B_up))  -- reference QuantLlamaMLP.triton_llama_mlp +
 * fusedmatmul_248_kernel (quant/fused_mlp.py:206-218, :84-168).  Both weight sets share
 * K, N, bits, groupsize; each has its own scales / qzeros / g_idx.
 */
int gptq_fused_mlp_f16(const void *x, int64_t ldx, const int32_t *qweight_gate,
                       const void *scales_gate, const int32_t *qzeros_gate,
                       const int32_t *g_idx_gate, const int32_t *qweight_up, const void *scales_up,
                       const int32_t *qzeros_up, const int32_t *g_idx_up, void *c, int64_t ldc,
                       int M, int K, int N, int bits, int groupsize, void *workspace,
                       size_t workspace_bytes, gptq_stream_t stream);

/*
 * The launch plan of the entries above as a host-only query: what the reference's autotuner would have chosen per shape
 * (quant/custom_autotune.py:76-102), here a static function of the arguments that a caller -- and a CPU test -- can read.  It
 * walks the entry's own dispatch code up to its FIRST dispatch call, launches nothing and touches no pointer; it honours the
 * current gptq_set_gemv_variant / gptq_set_split_k.
 *   entry      GPTQ_PLAN_ENTRY_AUTO: gptq_matmul248_f16 (nsets = 1) / gptq_fused_mlp_f16 (nsets = 2); _GEMV: gptq_gemv_f16;
 *              _SKINNY: gptq_skinny_f16; _ROWWAVE: the direct rowwave entries gptq_rmsnorm_matmul248_f16 / gptq_rmsnorm_fused_mlp_f16
 *              (GPTQ_PLAN_F_NORM; they have no M: M must be 1), gptq_matmul248_sorted_f16 / gptq_fused_mlp_sorted_f16
 *              (GPTQ_PLAN_F_X_PERM), gptq_rmsnorm_sorted_f16 (both flags).  Those two flags belong to this entry alone.
 *   flags      GPTQ_PLAN_F_G_IDX: a g_idx is passed (for every set); GPTQ_PLAN_F_NORM: a norm weight; GPTQ_PLAN_F_X_PERM: an x permutation
 *   workspace_bytes   what the call would bring (0: no workspace; the pointer counts as aligned)
 * Returns the kernel family of that first call (GPTQ_KERNEL_*; GPTQ_KERNEL_NONE: M = 0, nothing to launch) and fills
 * plan[GPTQ_PLAN_FIELDS] -- or the GPTQ_E_* the entry returns before any launch for such arguments (plan is zeroed; GPTQ_E_VARIANT
 * also for an unknown entry / flag, GPTQ_E_SHAPE for nsets outside 1 .. 2).  Fields a family does not have are 0:
 *   ROWWAVE (one launch per row) / ROWWAVE_MR / ROWWAVE_MFMA (all rows):  ROWS, UNIT = U packed rows (3-bit: 32-k blocks) in flight per
 *              wave, SPLIT_K, UPG_SHIFT = log2(units per group), -1 with one group
 *   GENERIC    ROWS, UNIT = nl (4 nl columns per workgroup), SPLIT_K = 1, NTILES, CHUNKS_PER_SLICE
 *   STREAM     ROWS of the pass, UNIT = units per stage, SPLIT_K, WAVES, XLDS (x staged in LDS), UPG_SHIFT, NTILES, CHUNKS_PER_SLICE
 *   TILE_GEMM  ROWS
 * The kernel may still decline at launch and hand the product to the next rung; the plan is that of the first call all the same.
 * Pinned over a grid of shapes, recorded from the dispatch calls themselves, by tests/test_host_gemv_plan.py.
 */
enum { GPTQ_PLAN_ENTRY_AUTO = 0, GPTQ_PLAN_ENTRY_GEMV = 1, GPTQ_PLAN_ENTRY_SKINNY = 2, GPTQ_PLAN_ENTRY_ROWWAVE = 3 };
enum { GPTQ_PLAN_F_G_IDX = 1, GPTQ_PLAN_F_NORM = 2, GPTQ_PLAN_F_X_PERM = 4 };
enum {
    GPTQ_KERNEL_NONE = 0,
    GPTQ_KERNEL_ROWWAVE = 1,       /* gemv_fast_dispatch (csrc/gemv.hip) */
    GPTQ_KERNEL_ROWWAVE_MR = 2,    /* gemv_rowwave_mr_dispatch */
    GPTQ_KERNEL_ROWWAVE_MFMA = 3,  /* gemv_rowwave_mfma_dispatch */
    GPTQ_KERNEL_GENERIC = 4,       /* gemv_generic_dispatch */
    GPTQ_KERNEL_STREAM = 5,        /* skinny_dispatch (csrc/skinny_mfma.hip) */
    GPTQ_KERNEL_TILE_GEMM = 6      /* gemm_dispatch (csrc/gemm_mfma.hip) */
};
enum {
    GPTQ_PLAN_ROWS = 0,
    GPTQ_PLAN_UNIT = 1,
    GPTQ_PLAN_SPLIT_K = 2,
    GPTQ_PLAN_WAVES = 3,
    GPTQ_PLAN_XLDS = 4,
    GPTQ_PLAN_UPG_SHIFT = 5,
    GPTQ_PLAN_NTILES = 6,
    GPTQ_PLAN_CHUNKS_PER_SLICE = 7,
    GPTQ_PLAN_FIELDS = 8
};
int gptq_gemv_plan_for_shape(int entry, int M, int K, int N, int bits, int groupsize, int nsets, int flags, size_t workspace_bytes, int *plan);

/*
 * dx[M,K] = dy[M,N] . deq(B)^T -- reference transpose_matmul248() +
 * transpose_matmul_248_kernel (quant/quant_linear.py:272-279, :191-258); the backward of
 * QuantLinearFunction (:294-301).
 */
int gptq_transpose_matmul248_f16(const void *dy, int64_t lddy, const int32_t *qweight,
                                 const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                                 void *dx, int64_t lddx, int M, int K, int N, int bits,
                                 int groupsize, gptq_stream_t stream);

/*
 * y = x * rsqrt(mean(x^2) + eps) * w, fp32 math, one rounding to fp16 -- reference
 * TritonLlamaRMSNorm.forward + rms_norm_fwd_fused (quant/triton_norm.py:50-67, :7-39).
 * Rows wider than 64 KiB are rejected like the reference (:59-60).
 */
int gptq_rmsnorm_f16(const void *x, int64_t ldx, const void *weight, void *y, int64_t ldy, int M,
                     int N, float eps, gptq_stream_t stream);

/* y[N] = W[N][K] . x (+ bias) for ONE row of x and a dense fp16 weight stored [out, in] (row stride ldw): the LM head of a decode
 * step -- the ordinary nn.Linear the reference's model ends in (llama_inference.py:119-127 -> HF generate), 262 MB per token for LLaMA-7B.
 * HBM-bound, hand-written (csrc/dense_gemv.hip): rows streamed non-temporally, x staged once per workgroup, fp32 accumulation.
 * norm_weight != NULL: x is RMS-normalised first (rms_norm_fwd_fused, quant/triton_norm.py:22-39, rounded to fp16 like the stand-alone
 * launch) -- the model's final norm folded into the same launch.  K % 8 == 0, K <= 65536. */
int gptq_dense_matvec_f16(const void *x, const void *weight, int64_t ldw, const void *bias, void *y, int N, int K, const void *norm_weight,
                          float norm_eps, gptq_stream_t stream);
/*
 * In-place rotate-half RoPE on the q and k slices of a fused qkv activation -- reference
 * triton_rotate_half_ + rotate_half_kernel (quant/fused_attn.py:61-93, :8-58).
 * qk points at element [0,0,0,0,0] of a [bsz, seq, 2, heads, head_dim] fp16 view whose
 * (bsz*seq) rows are row_stride elements apart; position_ids int64 [bsz, seq] with batch
 * stride pos_batch_stride.  cos/sin are computed on the fly in fp32 with theta = base.
 */
int gptq_rope_f16(void *qk, int64_t row_stride, const int64_t *position_ids,
                  int64_t pos_batch_stride, int bsz, int seq, int heads, int head_dim, float base,
                  gptq_stream_t stream);

/*
 * GPU packer -- reference QuantLinear.pack (quant/quant_linear.py:325-371), which runs on the
 * CPU upstream ("TODO: perform packing on GPU", llama.py:264).  weight fp32 [N, K] (nn.Linear
 * layout, already grid-valued), scales/zeros fp32 [N, G] as produced by gptq.py:226-228.
 * Bit-exact with the reference, including the unmasked OR and the zeros-1 wrap.
 */
int gptq_pack_f32(const float *weight, const float *scales, const float *zeros,
                  const int32_t *g_idx, int K, int N, int bits, int groupsize, int32_t *qweight,
                  int32_t *qzeros, void *scales_f16, gptq_stream_t stream);

/* 1 iff g_idx[k] == k / groupsize for all k (device-side check, writes one int32 to `out`). */
int gptq_g_idx_is_trivial(const int32_t *g_idx, int K, int groupsize, int32_t *out,
                          gptq_stream_t stream);

/*
 * Batch-1 decode-step helpers (extension over the reference, which does this part with torch ops
 * between its Triton kernels: triton_rotate_half_ + torch.cat of the KV cache + torch SDPA,
 * quant/fused_attn.py:126-155).  They read the current position from DEVICE memory and use a
 * preallocated cache, so a whole decode step can be captured in one hipGraph.
 *   qkv       fp16 [3, heads, head_dim] -- the fused qkv activation of ONE token; q is rotated in place
 *   position  int64 [1] on the device   -- index of the token being decoded (0-based)
 *   k_cache / v_cache  fp16 [t_max, heads*head_dim]; row `position` is written by rope_kv, rows
 *             0..position are read by attn.  head_dim must be 128 for gptq_decode_attn_f16.
 *   out       fp16 [heads*head_dim] = softmax(q.K^T * scale) V, fp32 math
 */
/*
 * W[K, N] fp16 = the dequantised weight exactly as the reference's kernel forms it on the fly:
 * fp16(q - z) * fp16 scale, one rounding (quant/quant_linear.py:114-128).  Any bits / g_idx.
 * Used by the Python layer for every batch above the weight-streaming kernels (prefill): the product is a plain
 * dense GEMM there, and dequantise-per-call (10-20 us for a LLaMA-7B layer) + library GEMM measures 1.12-1.39x
 * the fused tile kernel behind gptq_matmul248_f16.  A C caller with a BLAS at hand can do the same.
 */
int gptq_dequant_f16(const int32_t *qweight, const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                     void *w, int K, int N, int bits, int groupsize, gptq_stream_t stream);
/* the same with a leading dimension (ldw >= N halves): e.g. gate | up of an MLP side by side in ONE [K, 2N] matrix, so that the
 * pair is one library GEMM (quant/fused_mlp.py, prefill route). */
int gptq_dequant_ld_f16(const int32_t *qweight, const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                        void *w, int64_t ldw, int K, int N, int bits, int groupsize, gptq_stream_t stream);
/*
 * c[m][n] = fp16(silu(gate[m][n]) * up[m][n]), fp32 math -- the epilogue of the reference's fused MLP kernel
 * (quant/fused_mlp.py:160-165) as a pass of its own, for gate / up products that come out of a library GEMM.  N % 8 == 0,
 * leading dimensions multiples of 8 halves, 16-byte aligned pointers; c may alias gate.
 */
int gptq_silu_mul_f16(const void *gate, int64_t ldg, const void *up, int64_t ldu, void *c, int64_t ldc, int M, int N,
                      gptq_stream_t stream);

/*
 * Prefill route (M above the weight-streaming kernels): the layer is dequantised ONCE PER CALL into the workspace (reference
 * numerics fp16(q - z) * fp16 scale, any width, any g_idx -- act-order needs no gather of x here) and the dense product runs
 * through the hand-written tile GEMM of csrc/gemm8.hip (fp16 operands by LDS-DMA, v_mfma_f32_16x16x32_f16, fp32 accumulation,
 * one rounding, bias in the epilogue): same interface and results as gptq_matmul248_f16 / gptq_fused_mlp_f16 (reference
 * matmul248, quant_linear.py:263-269; fused MLP, fused_mlp.py:84-168).  The fused variant stacks gate and up as one [2N, K]
 * operand; ONE launch forms both products per tile and applies SiLU to the FP32 accumulators like the reference's kernel
 * (fused_mlp.py:160-165): no intermediate, no extra rounding.  gptq_set_prefill_route(0) -- and shapes the tile GEMM does not
 * serve (K % 128 != 0) -- take hipBLASLt instead (dlopen'ed at first use, GPTQ_E_LIBRARY when absent, bounded LRU of plans; the
 * gate | up product then leaves the library in FP32 in chunks of <= 8192 rows and SiLU * mul is a pass of its own).
 * workspace: gptq_prefill_workspace_bytes(M, K, N, nsets) bytes (nsets = 1 matmul, 2 fused MLP), 256-byte aligned;
 * GPTQ_E_WORKSPACE when smaller.  K % 32 == 0, N % 32 == 0 like everywhere; any M >= 0.
 */
size_t gptq_prefill_workspace_bytes(int M, int K, int N, int nsets);
int gptq_prefill_matmul_f16(const void *x, int64_t ldx, const int32_t *qweight, const void *scales, const int32_t *qzeros,
                            const int32_t *g_idx, const void *bias, void *y, int64_t ldy, int M, int K, int N, int bits,
                            int groupsize, void *workspace, size_t workspace_bytes, gptq_stream_t stream);
/* the backward product on the same route: dx[M, K] = dy[M, N] . deq(W)^T (reference transpose_matmul248,
 * quant_linear.py:272-279, kernel :191-258); interface of gptq_transpose_matmul248_f16 + the workspace (nsets = 1). */
int gptq_prefill_transpose_matmul248_f16(const void *dy, int64_t lddy, const int32_t *qweight, const void *scales,
                                         const int32_t *qzeros, const int32_t *g_idx, void *dx, int64_t lddx, int M, int K, int N,
                                         int bits, int groupsize, void *workspace, size_t workspace_bytes, gptq_stream_t stream);
int gptq_prefill_fused_mlp_f16(const void *x, int64_t ldx, const int32_t *qweight_gate, const void *scales_gate,
                               const int32_t *qzeros_gate, const int32_t *g_idx_gate, const int32_t *qweight_up,
                               const void *scales_up, const int32_t *qzeros_up, const int32_t *g_idx_up, void *c, int64_t ldc,
                               int M, int K, int N, int bits, int groupsize, void *workspace, size_t workspace_bytes,
                               gptq_stream_t stream);

/*
 * Act-order fast path (extension; the reference re-gathers g_idx, scales and zeros for every k row
 * in the kernel, quant/quant_linear.py:114-118).  With perm = stable argsort(g_idx), the re-sorted
 * qweight (gptq_act_order_repack, one-off at load; same shape as qweight) is a trivial-g_idx layer
 * applied to x[perm]: gptq_matmul248_sorted_f16 gathers x through perm on the scalar path and runs
 * the rowwave GEMV (one launch per row of x; M == 1 is the intended use).  scales / qzeros are the
 * checkpoint's own.  Valid when every group has exactly `groupsize` members (what gptq.py:210-216
 * produces) and groupsize % (32/bits) == 0; bits == 4 in this release (else GPTQ_E_VARIANT).
 */
int gptq_act_order_repack(const int32_t *qweight, const int32_t *perm, int K, int N, int bits,
                          int32_t *qweight_sorted, gptq_stream_t stream);
int gptq_matmul248_sorted_f16(const void *x, int64_t ldx, const int32_t *perm, const int32_t *qweight_sorted,
                              const void *scales, const int32_t *qzeros, const void *bias, void *y,
                              int64_t ldy, int M, int K, int N, int bits, int groupsize, void *workspace,
                              size_t workspace_bytes, gptq_stream_t stream);
/* The fused gate/up + SiLU of an act-order MLP: gate_proj and up_proj see the same input, hence the same Hessian
 * diagonal and the same act-order permutation (as q/k/v do, fused_attn.py:177-188) -- one perm, two re-sorted weight
 * sets, c = silu(x[perm].Wg') * (x[perm].Wu').  Same validity rules as gptq_matmul248_sorted_f16. */
int gptq_fused_mlp_sorted_f16(const void *x, int64_t ldx, const int32_t *perm, const int32_t *qweight_gate_sorted,
                              const void *scales_gate, const int32_t *qzeros_gate, const int32_t *qweight_up_sorted,
                              const void *scales_up, const int32_t *qzeros_up, void *c, int64_t ldc, int M, int K, int N,
                              int bits, int groupsize, void *workspace, size_t workspace_bytes, gptq_stream_t stream);
/* [RMSNorm -> act-order QuantLinear] (qweight_up_sorted == NULL) or [RMSNorm -> act-order gate/up + SiLU] of one decode
 * token in ONE launch: the kernel gathers x and the norm weight through perm and normalises what it gathered
 * (sum(x^2) does not depend on the order).  M == 1, 4-bit, groups of >= 64. */
int gptq_rmsnorm_sorted_f16(const void *x, const void *norm_weight, float eps, const int32_t *perm, const int32_t *qweight_sorted,
                            const void *scales, const int32_t *qzeros, const int32_t *qweight_up_sorted, const void *scales_up,
                            const int32_t *qzeros_up, const void *bias, void *y, int K, int N, int bits, int groupsize,
                            void *workspace, size_t workspace_bytes, gptq_stream_t stream);

/*
 * [RMSNorm -> QuantLinear] and [RMSNorm -> fused gate/up] of a decoder layer as ONE launch, M == 1
 * (TritonLlamaRMSNorm.forward followed by QuantLinear.forward / triton_llama_mlp; reference
 * quant/triton_norm.py:50-67 + quant/quant_linear.py:373-377 / quant/fused_mlp.py:206-218).
 * x fp16 [K] is normalised on the fly with the arithmetic of rms_norm_fwd_fused (fp32, one fp16
 * rounding) and never written back.  Returns GPTQ_E_VARIANT when the shape needs the generic
 * kernels (act-order, 3-bit, bits != 4, odd groups): call gptq_rmsnorm_f16 + gptq_matmul248_f16.
 */
int gptq_rmsnorm_matmul248_f16(const void *x, const void *norm_weight, float eps, const int32_t *qweight,
                               const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                               const void *bias, void *y, int K, int N, int bits, int groupsize,
                               void *workspace, size_t workspace_bytes, gptq_stream_t stream);
int gptq_rmsnorm_fused_mlp_f16(const void *x, const void *norm_weight, float eps, const int32_t *qweight_gate,
                               const void *scales_gate, const int32_t *qzeros_gate,
                               const int32_t *g_idx_gate, const int32_t *qweight_up, const void *scales_up,
                               const int32_t *qzeros_up, const int32_t *g_idx_up, void *c, int K, int N,
                               int bits, int groupsize, void *workspace, size_t workspace_bytes,
                               gptq_stream_t stream);

int gptq_decode_rope_kv_f16(void *qkv, const int64_t *position, void *k_cache, void *v_cache, int heads,
                            int head_dim, int t_max, float base, gptq_stream_t stream);
size_t gptq_decode_attn_workspace_bytes(int heads, int head_dim, int t_max);
int gptq_decode_attn_f16(const void *q, const void *k_cache, const void *v_cache, const int64_t *position,
                         void *out, void *workspace, size_t workspace_bytes, int heads, int head_dim,
                         int t_max, float scale, gptq_stream_t stream);

/* gptq_decode_rope_kv_f16 + gptq_decode_attn_f16 as ONE launch (q is rotated internally, the qkv
 * buffer is left untouched); the workspace (same size query; 16-byte aligned) must be zero on first use -- its
 * trailing [heads] uint32 arrival tickets are restored to zero by the kernel.  Round 6: a streaming kernel -- one
 * workgroup per head walks the whole history up to ~768 tokens (no merge at all), at most gptq_decode_attn_splits()
 * splits with an arrival ticket beyond (see "round 6" below). */
int gptq_decode_attn_fused_f16(const void *qkv, const int64_t *position, void *k_cache, void *v_cache, void *out,
                               void *workspace, size_t workspace_bytes, int heads, int head_dim, int t_max,
                               float base, float scale, gptq_stream_t stream);
/* The same launch with {cos, sin} read from a table gptq_rope_table_f32 filled once ([t_max][head_dim / 2][2] fp32, the identical
 * instruction sequence: bit-identical results): the accurate-libm range reduction leaves the per-token critical path. */
int gptq_rope_table_f32(float *table, int t_max, int head_dim, float base, gptq_stream_t stream);
int gptq_decode_attn_fused_table_f16(const void *qkv, const int64_t *position, void *k_cache, void *v_cache, void *out, void *workspace,
                                     size_t workspace_bytes, int heads, int head_dim, int t_max, float base, float scale,
                                     const float *rope_table, gptq_stream_t stream);

/* ---- stripe16: the batch-1 decode matvec WITHOUT a K split, on a load-time repacked copy (csrc/stripe.hip) --------
 * Replaces, for M == 1, the launch of matmul_248_kernel (quant/quant_linear.py:263-269) / fusedmatmul_248_kernel
 * (quant/fused_mlp.py:206-218) on a layout the library owns: the checkpoint buffers are repacked ONCE at load time
 * (the reference has no counterpart; its load path ends at load_state_dict, llama_inference.py:57-60) into
 *   R   uint32 [N/16][K/128][nsets][64][4]  (4-bit) every workgroup's 16 columns contiguous, 1 KiB per wave load, fields
 *                                            re-ordered for a one-shift unpack (see csrc/stripe.hip)
 *   tab half2  [N/16][nsets][G][16]          {scale, zero + 1} per (group, column)
 * stored back to back in ONE buffer of gptq_stripe_bytes() bytes (0 = shape not eligible: bits in {2, 3, 4, 8}; K a multiple of
 * the row block = 256 / 128 / 128 / 64 k and at most 24576 / 24576 / 24576 / 22528; groupsize a power-of-two multiple of a quarter
 * of the row block that divides K, or >= K).  For 8 and 2 bits the same geometry holds with 32 / bits k per word, for 3 bits a lane
 * holds its 32 k in three words ([N/16][K/128][nsets][64][3]); see csrc/stripe.hip.  The
 * checkpoint buffers are not modified and stay the owner of the state_dict.  nsets == 2 packs gate and up together and the
* matvec returns silu(x Wg) * (x Wu).  1 <= M <= 4 rows of x (row strides ldx / ldy) cost the same weight stream as one: the
 * MFMA computes four rows anyway; 5 <= M <= 8 / 16 run two / four MFMA row groups on the same unpacked words while M rows of x
 * fit in LDS (K <= ~9200 / ~4600, else GPTQ_E_VARIANT: the caller takes the weight-streaming MFMA kernel).  M == 1 only: norm_weight != NULL fuses the RMSNorm of x (rms_norm_fwd_fused,
 * quant/triton_norm.py:22-39) in front; perm != NULL (uint16 [K]: the same permutation gptq_act_order_repack takes, narrowed -- every
 * workgroup reads all of it, so its width is load traffic) reads x through a permutation (an act-order layer whose qweight rows were
 * sorted by group with gptq_act_order_repack BEFORE gptq_stripe_repack).  No workspace, no atomics: results are bit-identical
 * run to run. */
size_t gptq_stripe_bytes(int K, int N, int bits, int groupsize, int nsets);
int gptq_stripe_repack(const int32_t *qweight, const void *scales, const int32_t *qzeros, const int32_t *qweight_up, const void *scales_up,
                       const int32_t *qzeros_up, void *stripes, size_t stripes_bytes, int K, int N, int bits, int groupsize,
                       gptq_stream_t stream);
int gptq_stripe_matvec_f16(const void *x, int64_t ldx, const void *stripes, size_t stripes_bytes, const void *bias, void *y, int64_t ldy, int M,
                           int K, int N, int bits, int groupsize, int nsets, const void *norm_weight, float norm_eps, const uint16_t *perm,
                           gptq_stream_t stream);
/* The same matvec with the fp32 sums stored unrounded: the per-rank PARTIAL of a row-(K-)sharded layer (BASELINE config 5,
 * quant/tensor_parallel.py) -- the shards are summed by ONE all-reduce and rounded to fp16 once, like the unsharded layer.
 * y_partial is fp32 [nsets][N]: with nsets == 2 the gate and the up sums are stored separately (no SiLU: it needs the
 * complete sums). */
int gptq_stripe_matvec_partial_f32(const void *x, const void *stripes, size_t stripes_bytes, float *y_partial, int K, int N, int bits,
                                   int groupsize, int nsets, const uint16_t *perm, gptq_stream_t stream);
/* The same for 1 <= M <= 4 rows of x (row stride ldx): y_partial is fp32 [M][nsets][N] -- the row groups of the decode kernel cost the
 * weight stream of one row, so a K-shard of a small decode batch keeps the one-rounding-after-the-reduce order of M = 1 (trivial g_idx
 * only: gather x[:, perm] first for a group-sorted act-order image). */
int gptq_stripe_matmul_partial_f32(const void *x, int64_t ldx, const void *stripes, size_t stripes_bytes, float *y_partial, int M, int K, int N,
                                   int bits, int groupsize, int nsets, gptq_stream_t stream);
/* Batches on the same image (csrc/stripe_mm.inc).  1 <= M <= 128 (to 256 in passes of 128): 16-row MFMA tiles (v_mfma_f32_16x16x32_f16) on exactly
 * dequantised q - z, fp32 group scales; either one launch (a stripe x whole K per workgroup, x streamed through LDS) or K slices
 * (128 columns x one slice per workgroup) that meet through fp32 partial tiles in `workspace` and a reduce kernel (summed in
 * slice order: bit-reproducible; no atomics).  Every layer with a stripe image (bits 2 / 3 / 4 / 8): groups of at least a row block
 * keep q - z exact and scale the fp32 accumulator; smaller groups multiply by the lane's fp16 scale before the MFMA (one rounding, the
 * reference's own dequantisation, quant_linear.py:128); GPTQ_E_VARIANT when there is no image (callers fall back to gptq_matmul248_f16).  The workspace
 * (gptq_query(GPTQ_Q_STRIPE_MM_WORKSPACE_BYTES), 256-byte aligned) is pure scratch for the partial tiles: no initialisation, no state
 * between launches; do not share it between launches that may overlap, nor with the zero-invariant split-K workspace of the
 * rowwave kernels.  129 <= M <= gptq_set_stripe_gemm_max_rows() (default 2048; groups of at least a row block, bits 3 / 4 / 8): ONE launch of
 * the 2-D tiled fused-dequantise GEMM (stripe_gemm_kernel: 128 x 128 tiles, weights stay packed, x through LDS) -- no per-call
 * dequantise pass; round 5: while the tiles cover at most half the chip (N = 4096: up to 512 rows) K is sliced over the row tiles too
 * (partial tiles in `workspace` + the reduce kernel, as below 129 rows).  Round 6: 17 <= M <= 128 of a 4-bit layer whose stripes need two or three
 * rounds of workgroups (N = 8192 .. 12288; K <= 8192) and of the gate | up pair of such a shape run the loader / consumer kernel (stripe_mmr_kernel:
 * two waves per workgroup stream x into an LDS ring by LDS-DMA, six only read A fragments out of it and run the MFMAs on weights unpacked in their
 * registers; the pair's consumers split by set) -- one launch, no workspace; a long K on one round of stripes (N <= 4096, K > 6144) runs its K-sliced
 * form: fp32 rows per slice in `workspace` + a combine launch (slice order, one rounding).  Same arithmetic and result conventions as the tiles above.
 * Reference semantics: quant/quant_linear.py:103-137, :415-419; nsets = 2: quant/fused_mlp.py:128-168 (no bias). */
int gptq_stripe_matmul_f16(const void *x, int64_t ldx, const void *stripes, size_t stripes_bytes, const void *bias, void *y, int64_t ldy, int M,
                           int K, int N, int bits, int groupsize, int nsets, void *workspace, size_t workspace_bytes, gptq_stream_t stream);

/* ---- one-shot all-reduce for the row-sharded layout (BASELINE config 5; csrc/p2p.hip) ------------------------------
 * New functionality (the reference has no collective: llama.py:328-382 is layer placement).  The fp32 partials of a
 * K-sharded QuantLinear are 32-176 KB at batch 1 -- latency-bound -- and MI355X's xGMI is a full mesh, so every rank
 * WRITES its partial into all peers (memory mapped through HIP IPC), flags, and sums the P slots locally in rank order:
 * one hop instead of the 2 (P - 1) of a ring, bit-identical results on every rank, fp16 rounding (+ bias) fused.
 *   gptq_p2p_create   allocates this rank's exchange buffer (gptq_p2p_buffer_bytes: two slot sets [world][n_max] fp32 +
 *                     flags + per-workgroup epoch counters, zeroed) and exports its 64-byte IPC handle; the caller ships
 *                     the handle to the other ranks (any channel, e.g. torch.distributed.all_gather_object)
 *   gptq_p2p_open     maps a peer's buffer into this process (hipIpcOpenMemHandle; needs HSA_ENABLE_IPC_MODE_LEGACY=0)
 *   gptq_p2p_allreduce_f32  peer_buffers = HOST array of `world` pointers, [rank] = own buffer; n % 4 == 0, n <= n_max;
 *                     writes y_f16 = fp16(sum) (+ bias) or, when y_f32 != NULL, the fp32 sum.  All ranks must issue the same
 *                     sequence of calls.  hipGraph-capturable (the epoch lives in device memory).
 *   gptq_p2p_status   0, or 1 + the rank a workgroup gave up waiting for (every spin is bounded). */
size_t gptq_p2p_buffer_bytes(int world, int n_max);
int gptq_p2p_create(int world, int n_max, void **buffer, void *ipc_handle_64);
int gptq_p2p_open(const void *ipc_handle_64, void **buffer);
int gptq_p2p_close(void *buffer, int opened);
int gptq_p2p_status(void *own_buffer, int world, int n_max, gptq_stream_t stream);
int gptq_p2p_allreduce_f32(const float *partial, void *const *peer_buffers, int rank, int world, int n, int n_max, void *y_f16, float *y_f32,
                           const void *bias, gptq_stream_t stream);
/* partial = [2][n_half] fp32, the gate | up partials of a K-sharded fused MLP (gptq_stripe_matvec_partial_f32 with nsets = 2):
 * y_f16[n_half] = fp16(silu(sum gate) * sum up) -- the epilogue of fusedmatmul_248_kernel (quant/fused_mlp.py:160-166), after the reduce. */
int gptq_p2p_allreduce_silu_mul_f32(const float *partial, void *const *peer_buffers, int rank, int world, int n_half, int n_max, void *y_f16,
                                    gptq_stream_t stream);

/* ---- Prepared layers: the ONE call site of the product ------------------------------------------------------------------
 * The reference reaches its kernels through a single call, matmul248(input, qweight, scales, qzeros, g_idx, bits, maxq)
 * (quant/quant_linear.py:263-269) behind QuantLinear.forward (:373-377) -- and fusedmatmul_248 behind QuantLlamaMLP
 * (quant/fused_mlp.py:203-218) -- with an autotuner that picks a kernel per M (custom_autotune.py).  Here a layer is PREPARED once
 * (load time): g_idx is inspected on the host (0 trivial / 1 regular act-order / 2 irregular), the stripe16 image -- of the
 * group-sorted rows plus the permutation for a regular act-order layer -- is built into the caller's image buffer, and
 * gptq_layer_forward() contains the whole M -> kernel table: decode matvec (M = 1, the headline path), row groups (M <= 8),
 * 16-row MFMA tiles (M <= 128), the prefill tile GEMM / library route above, the checkpoint-layout kernels for whatever has no
 * image.  A non-Python consumer binds exactly these entries and gets the product's speed.
 *
 * Memory stays the caller's: `image` (gptq_layer_image_bytes, 256-byte aligned; NULL = no derived copies, checkpoint-layout
 * kernels only), `workspace` (gptq_layer_workspace_bytes(); its first gptq_query(GPTQ_Q_WORKSPACE_BYTES) bytes must be ZERO on
 * first use and are left zero by every call -- one per stream that may run concurrently), `scratch` (gptq_layer_scratch_bytes(layer,
 * M): transient, may be NULL -- forward then takes a slower route that needs none).  The checkpoint buffers are borrowed and must
 * outlive the handle; the handle is a small host object.  gptq_layer_prepare / _inspect synchronise the stream (load time);
 * gptq_layer_forward only enqueues and is hipGraph-capturable.  nsets = 2 (qweight_up != NULL): y = silu(x Wg) * (x Wu).
 */
typedef struct gptq_layer gptq_layer_t;
int gptq_layer_inspect(const int32_t *g_idx, int K, int groupsize, gptq_stream_t stream);   /* 0 / 1 / 2, or GPTQ_E_* */
size_t gptq_layer_image_bytes(int K, int N, int bits, int groupsize, int nsets, int kind);
int gptq_layer_prepare(gptq_layer_t **layer, const int32_t *qweight, const void *scales, const int32_t *qzeros, const int32_t *g_idx,
                       const void *bias, const int32_t *qweight_up, const void *scales_up, const int32_t *qzeros_up,
                       const int32_t *g_idx_up, int K, int N, int bits, int groupsize, void *image, size_t image_bytes,
                       gptq_stream_t stream);
void gptq_layer_destroy(gptq_layer_t *layer);
int gptq_layer_kind(const gptq_layer_t *layer);
int gptq_layer_stripe_image(const gptq_layer_t *layer, const void **stripe, size_t *stripe_bytes, const uint16_t **perm16);
/* Memory mode (reference README.md:23-29 quotes 4891 MiB for 7B 4-bit g128: ONE copy of the packed weights): after this call the
 * caller may free qweight / scales / qzeros -- the stripe16 image is a bijection of them.  Trivial or (round 4) regular act-order g_idx --
 * its image holds the group-sorted rows, the permutation and its inverse; g_idx itself (K ints) stays borrowed --, any width, and an
 * image (GPTQ_E_VARIANT otherwise, nothing changes).  Routes that read the checkpoint layout (prefill, fall-backs) then rebuild it
 * from the image into `scratch` per call; gptq_layer_unpack_checkpoint reproduces one weight set bit-exactly (state_dict()). */
int gptq_layer_release_checkpoint(gptq_layer_t *layer);
int gptq_layer_unpack_checkpoint(const gptq_layer_t *layer, int set, int32_t *qweight, void *scales, int32_t *qzeros, gptq_stream_t stream);
size_t gptq_layer_workspace_bytes(void);
size_t gptq_layer_scratch_bytes(const gptq_layer_t *layer, int M);
/* every fall-back's needs at once: the scratch to retry with when forward() answers GPTQ_E_WORKSPACE (a kernel of the fast route declined at launch) */
size_t gptq_layer_fallback_scratch_bytes(const gptq_layer_t *layer, int M);
int gptq_layer_forward(const gptq_layer_t *layer, const void *x, int64_t ldx, void *y, int64_t ldy, int M, void *workspace,
                       size_t workspace_bytes, void *scratch, size_t scratch_bytes, gptq_stream_t stream);
/* The M -> kernel table of gptq_layer_forward as a host-only query (no launch, no GPU needed): the kernel family a batch of M rows takes,
 * assuming the caller passes gptq_layer_scratch_bytes() of scratch.  It replaces what the reference's Autotuner decides at run time
 * (quant/custom_autotune.py:76-102) by something a caller can read.  A kernel may still decline at launch (LDS limits) and hand the
 * batch to the next rung of the ladder.  kind: the value of gptq_layer_inspect(); has_image: an image was given to gptq_layer_prepare. */
enum {
    GPTQ_ROUTE_STRIPE_DECODE = 1,        /* stripe16 decode kernel (M = 1) / its row groups (2 .. 8 rows); wide layers: C stripes per workgroup (round 5) */
    GPTQ_ROUTE_STRIPE_TILES = 2,         /* 16-row MFMA tiles on the image, up to 128 rows (csrc/stripe_mm.inc) */
    GPTQ_ROUTE_STRIPE_GEMM = 3,          /* fused-dequantise tile GEMM on the image, 129 .. gptq_set_stripe_gemm_max_rows() rows (see there) */
    GPTQ_ROUTE_DENSE_TILE_GEMM = 4,      /* dequantise per call + the tile GEMM of csrc/gemm8.hip */
    GPTQ_ROUTE_DENSE_LIBRARY = 5,        /* dequantise per call + hipBLASLt */
    GPTQ_ROUTE_CHECKPOINT_KERNELS = 6    /* rowwave / stream / generic kernels on the checkpoint layout */
};
int gptq_layer_route_for_shape(int M, int K, int N, int bits, int groupsize, int nsets, int kind, int has_image);
int gptq_layer_route_for(const gptq_layer_t *layer, int M);

/* ---- Batched decode (round 5) --------------------------------------------------------------------------------------------
 * The reference serves every batch with the one kernel (matmul248 masks M only, quant/quant_linear.py:263-269, :373-377) and HF
 * `generate` drives it with [B, 1] steps, left-padded prompts and per-row position_ids (llama_inference.py:119-127).  The entries
 * below are what a graph-captured decode step of B <= 16 sequences is made of (quant/decode.py DecodeEngine(batch = B)):
 *
 * gptq_layer_decode_f16      y[M][N] = residual[M][..] + layer(rmsnorm(x[M][K]))   (norm_weight / residual may be NULL; 1 <= M <= 128)
 *     one decoder block = four of these (input norm -> qkv, o_proj + residual, post-attention norm -> gate/up with SiLU, down_proj
 *     + residual: quant/fused_attn.py:117-161, quant/fused_mlp.py:203-218 between HF's norms and adds).  The decode kernel takes norm
 *     and residual into its own launch up to 4 rows (8 on shapes one round of workgroups covers); the 16-row MFMA tiles take the
 *     residual into their epilogue, the norm then is one launch into `scratch` (gptq_layer_decode_scratch_bytes).  The residual is
 *     added to the ROUNDED product (fp16(fp16(acc) + r)), as the module chain does it (one fp16 tensor add).  y must not alias x.
 * gptq_decode_attn_batch_f16  the fused RoPE + KV append + single-query attention launch (gptq_decode_attn_fused_table_f16) for B rows:
 *     positions[b] (negative = idle row), qkv row b at qkv + b ldq, out row b at out + b ldo, cache slice b at k_cache + b t_max heads 128;
 *     out_perm != NULL: element k of an output row is stored at out_perm[k] (see "Producer-side permutation" below).
 * gptq_dense_matmat_f16       y[M][N] = rmsnorm(x)[M][K] . W[N][K]^T, M <= 16, ONE pass over the dense fp16 weight (the LM head).
 * gptq_add_rows_f16           y = fp16(y + r), row by row.
 */
size_t gptq_layer_decode_scratch_bytes(const gptq_layer_t *layer, int M);
int gptq_layer_decode_f16(const gptq_layer_t *layer, const void *x, int64_t ldx, void *y, int64_t ldy, int M, const void *norm_weight,
                          float norm_eps, const void *residual, int64_t ldr, void *workspace, size_t workspace_bytes, void *scratch,
                          size_t scratch_bytes, gptq_stream_t stream);
/* Round 6: gptq_layer_decode_f16 that leaves the NEXT RMSNorm's rows behind when that is free.  A decode batch of 9 .. 16 rows runs a long-K
 * layer (LLaMA's down_proj) as K slices of the 16-row tiles + a combine launch; that launch owns whole rows of y, so it also writes
 * h[M][ldh] = rmsnorm(y) * next_norm_weight -- bit for bit what gptq_rmsnorm_f16 writes (triton_norm.py:22-39 between down_proj and the next block's
 * qkv_proj: llama modeling's input_layernorm) -- and sets *h_written = 1: the consumer runs without its norm, one launch less per decoder block
 * (at 16 rows the norm fused into the consumer's launch costs more than a launch: every workgroup would normalise all rows itself).  Every
 * other route behaves exactly like gptq_layer_decode_f16, leaves h untouched and sets *h_written = 0.  1 <= M <= 16 for the fusion. */
int gptq_layer_decode_next_norm_f16(const gptq_layer_t *layer, const void *x, int64_t ldx, void *y, int64_t ldy, int M, const void *norm_weight,
                                    float norm_eps, const void *residual, int64_t ldr, const void *next_norm_weight, float next_norm_eps, void *h,
                                    int64_t ldh, int *h_written, void *workspace, size_t workspace_bytes, void *scratch, size_t scratch_bytes,
                                    gptq_stream_t stream);
size_t gptq_decode_attn_batch_workspace_bytes(int batch, int heads, int head_dim, int t_max);
int gptq_decode_attn_batch_f16(const void *qkv, int64_t ldq, const int64_t *positions, void *k_cache, void *v_cache, void *out, int64_t ldo,
                               void *workspace, size_t workspace_bytes, int batch, int heads, int head_dim, int t_max, float base, float scale,
                               const float *rope_table, const int32_t *out_perm, gptq_stream_t stream);
/* Producer-side permutation (round 5): the reference gathers g_idx / scales / zeros per k row in its kernel (quant_linear.py:114-118); here a regular
 * act-order layer runs on the image of its group-sorted rows, which needs x in sorted order.  At M = 1 the decode kernel gathers x itself; where the
 * PRODUCER of x is one of our launches it can write x sorted instead: out_perm above (attention -> o_proj) and gptq_stripe_matvec_perm_out_f16
 * (gate/up + SiLU -> down_proj) store element n at perm[n], perm = gptq_layer_inverse_perm() of the consuming layer, which then runs the trivial
 * kernel (perm = NULL).  NULL = natural order. */
int gptq_layer_inverse_perm(const gptq_layer_t *layer, const int32_t **invperm32);
int gptq_stripe_matvec_perm_out_f16(const void *x, int64_t ldx, const void *stripes, size_t stripes_bytes, const void *bias, void *y, int64_t ldy, int M,
                                    int K, int N, int bits, int groupsize, int nsets, const void *norm_weight, float norm_eps, const uint16_t *perm,
                                    const int32_t *y_perm, gptq_stream_t stream);
int gptq_dense_matmat_f16(const void *x, int64_t ldx, const void *weight, int64_t ldw, const void *bias, void *y, int64_t ldy, int M, int N,
                          int K, const void *norm_weight, float norm_eps, gptq_stream_t stream);
int gptq_add_rows_f16(void *y, int64_t ldy, const void *r, int64_t ldr, int M, int N, gptq_stream_t stream);

/* ---- round 6: the decode attention as a STREAMING launch whose splits are merged by the NEXT launch ------------------------------------------
 * Replaces F.scaled_dot_product_attention over the grown cache (quant/fused_attn.py:142-155) for one new token per row.  The launch behind every
 * gptq_decode_attn_* entry cuts a row's history into at most gptq_decode_attn_splits() ranges chosen from the row's length at run time; a split is
 * one workgroup that walks its range with an online softmax and ends with a record per head: {M, den} in fp32 and its normalised partial
 * output o[128] in fp16 (one split: o IS the output row).  The entries above merge
 * the records themselves (one split: nothing to merge; several: arrival ticket, last split merges).  The pair below leaves them to the consumer:
 *
 * gptq_decode_attn_split_f16   RoPE + KV append + attention like gptq_decode_attn_batch_f16, but NO output row: the records stay in `workspace`
 *                              ([batch][S][heads * 128] fp16 partial outputs | [batch][S][heads] fp32 {M, den}; S = gptq_decode_attn_splits()).
 * gptq_layer_decode_attn_f16   y = residual + layer(x), where x is the merge of those records, formed while the decode kernel stages x (the
 *                              kernel boundary is the hand-off between the splits' workgroups).  One row, a layer with a trivial g_idx and a
 *                              stripe16 image, K = heads * 128 (o_proj of a batch-1 decode step); GPTQ_E_VARIANT otherwise --
 *                              gptq_layer_decode_attn_supported() answers 1 / 0 ahead of time.  Bit-identical to
 *                              gptq_decode_attn_batch_f16 + gptq_layer_decode_f16 at the same tokens_per_split.
 * tokens_per_split <= 0: the library's default for the mode; both calls of a pair must pass the same value (and the same t_max / batch). */
int gptq_decode_attn_splits(int batch, int heads, int head_dim, int t_max);
int gptq_decode_attn_split_f16(const void *qkv, int64_t ldq, const int64_t *positions, void *k_cache, void *v_cache, void *workspace,
                               size_t workspace_bytes, int batch, int heads, int head_dim, int t_max, float base, float scale, const float *rope_table,
                               int tokens_per_split, gptq_stream_t stream);
int gptq_layer_decode_attn_supported(const gptq_layer_t *layer, int batch, int heads, int head_dim);
int gptq_layer_decode_attn_f16(const gptq_layer_t *layer, const void *attn_workspace, size_t attn_workspace_bytes, const int64_t *positions, int batch,
                               int heads, int head_dim, int t_max, int tokens_per_split, void *y, int64_t ldy, const void *residual, int64_t ldr,
                               gptq_stream_t stream);

/* ---- fp8 KV cache: the decode attention over e4m3 rows with one power-of-two exponent per (token, head) (csrc/decode_attn_kv8.hip) -------------
 * At depth a decode step is the stream of the K/V cache (the reference grows it by torch.cat and reads all of it per token, quant/fused_attn.py:
 * 142-155); this format halves those bytes.  One cache (K or V) of `slots` sequences is two arrays:
 *     k8 / v8       uint8 [slot][t_max][heads * 128]   OCP e4m3fn bytes q_i
 *     kexp / vexp   int8  [slot][t_max][heads]         one exponent e per (token, head); the stored head row means q_i * 2^e
 * Quantising a head row r[0 .. 128) of fp16 values (for K: the bits the fp16 cache would hold -- rotated, rounded to fp16):
 *     amax = max |r_i|;  e = 0 when amax == 0, else the smallest integer with amax * 2^-e <= 448 -- with amax = m * 2^x, m in [0.5, 1): e = x - 9
 *     when m <= 0.875, else x - 8 -- so e lies in [-32, 8] and amax * 2^-e in (224, 448];
 *     q_i = RNE_e4m3(r_i * 2^-e): the scaling is exact, the rounding is to nearest even (subnormals of e4m3 included) and never overflows.
 * In PyTorch on the CPU: torch.ldexp(r.float(), -e).to(torch.float8_e4m3fn) -- that restatement (tests/kv8_ref.py) is the specification.  Rows
 * with NaN / inf are outside the contract; they cannot fault (no index depends on data).
 *
 * gptq_decode_attn_batch_kv8_f16   gptq_decode_attn_batch_f16 on such a cache: out[b, h] = softmax(scale q^ K^T) V^ over rows 0 .. positions[b],
 *     q^ the rotated fp16 query, K^ / V^ the dequantised rows INCLUDING row positions[b]: the new token is rotated, quantised, attended to in
 *     its quantised form and appended (bytes and exponents), so a step is a function of the cache alone.  Everything else -- idle rows
 *     (positions[b] < 0 or >= t_max: nothing read or written), the run-time split count, the deterministic merge, out_perm, the workspace of
 *     gptq_decode_attn_batch_workspace_bytes -- is that entry's.  tokens_per_split <= 0: the library's default (one split up to 768 tokens).
 *     Validated before the launch: GPTQ_E_NULL (any pointer but rope_table / out_perm), GPTQ_E_SHAPE (batch outside 1 .. 65535, heads < 1,
 *     head_dim != 128, t_max < 1, (t_max + 1024) heads 128 >= 2^31, ldq < 3 heads 128, ldo < heads 128), GPTQ_E_ALIGN (qkv / k8 / v8 / workspace
 *     16 bytes, positions and rope_table 8, out_perm 4, out 2, ldq / ldo multiples of 8), GPTQ_E_WORKSPACE.
 * gptq_kv8_store_f16               for each of nseq <= 16 segments {row0 (ignored), rows, start, slot}: rows start .. start + rows - 1 of slot
 *     `slot` of an fp16 cache k16 / v16 ([t_max][heads 128] per slot, slots slot_stride ELEMENTS apart) -> the same rows of the same slot of
 *     the fp8 cache ([slot][t_max][..] dense), by the rule above.  One launch, no atomics; nothing outside the segments is written.  What the
 *     prompt paths run behind gptq_prompt_attn_f16 / gptq_prompt_attn_batch_f16 on an fp16 staging cache.  `segs` is a HOST array, passed by
 *     value.  GPTQ_E_NULL (any pointer), GPTQ_E_SHAPE (nseq outside 1 .. 16, heads < 1, head_dim != 128, t_max < 1, slot_stride < t_max heads
 *     128, a segment with rows <= 0, start < 0, start + rows > t_max or slot < 0), GPTQ_E_ALIGN (k16 / v16 / k8 / v8 16 bytes, slot_stride a
 *     multiple of 8). */
int gptq_decode_attn_batch_kv8_f16(const void *qkv, int64_t ldq, const int64_t *positions, void *k8, void *v8, void *kexp, void *vexp, void *out,
                                   int64_t ldo, void *workspace, size_t workspace_bytes, int batch, int heads, int head_dim, int t_max, float base,
                                   float scale, const float *rope_table, const int32_t *out_perm, int tokens_per_split, gptq_stream_t stream);

/* ---- prompt prefill: causal attention of a chunk of tokens over the decode engine's own cache (csrc/prompt_attn.hip) ----------------------------
 * Replaces, for a prompt, what QuantLlamaAttention.forward does between qkv_proj and o_proj (quant/fused_attn.py:126-158: triton_rotate_half_ on q and
 * k, torch.cat onto the past, F.scaled_dot_product_attention with is_causal) on the cache layout of the decode entries above: `rows` consecutive
 * tokens of ONE sequence at positions start .. start + rows - 1, their fused projection qkv [rows][3 heads 128] (q | k | v, rows ldq apart, left
 * untouched), the sequence's cache slices k_cache / v_cache [t_max][heads 128].  The rotated k rows and the v rows are written to cache rows
 * start .. start + rows - 1, bit-identical to what gptq_decode_rope_kv_f16 writes for the same row and position; out[r][h] = softmax(scale q_r .
 * K[0 .. start + r]) V[0 .. start + r] (fp32 accumulation, one fp16 rounding, rows ldo apart).  Rows below start are read as earlier calls left
 * them, rows at and beyond start + rows are never touched.  Flash-style on the matrix core (no score matrix in memory, no atomics: bit-identical
 * from run to run); rope_table = NULL computes the trig in the kernel, bit-identical to the table of gptq_rope_table_f32.  start is a host value
 * (prefill is not graph-captured).  The workspace holds one fp16 copy of the rotated q.  head_dim must be 128. */
size_t gptq_prompt_attn_workspace_bytes(int rows, int heads, int head_dim, int t_max);
int gptq_prompt_attn_f16(const void *qkv, int64_t ldq, int rows, int64_t start, void *k_cache, void *v_cache, void *out, int64_t ldo,
                         void *workspace, size_t workspace_bytes, int heads, int head_dim, int t_max, float base, float scale,
                         const float *rope_table, gptq_stream_t stream);

/* The same for up to 16 SEGMENTS at once -- chunks of different sequences, of any lengths and start positions -- that share one packed qkv / out
 * matrix and one cache allocation: what a batch of prompts needs to enter the decode engine in one pass over the weights.  Segment i is `rows`
 * consecutive tokens of one sequence at positions start .. start + rows - 1; its projection rows are qkv + (row0 + r) ldq, its output rows
 * out + (row0 + r) ldo, its cache slices k_cache / v_cache + slot * slot_stride ([t_max][heads 128] each, slot_stride in elements: the engine's
 * [batch][t_max][heads 128] cache with slot_stride = t_max heads 128).  Per segment the contract -- and every bit of the output rows and the cache
 * rows -- is that of the single-sequence entry on that segment alone: one kernel body serves both, in TWO launches however many segments there
 * are.  The order of the table does not matter (the library issues long key ranges first).  Rows of qkv / out that no segment covers are neither
 * read nor written, nor are cache slices that no segment names.  `segs` is a HOST array: it is validated, then passed to the kernels by value in
 * the launch arguments (256 bytes) -- the library allocates nothing, copies nothing, never synchronises, and the caller may reuse the array at
 * once.  total_rows = rows of qkv / out; the workspace is that of the single-sequence entry for total_rows, which may exceed t_max.
 * GPTQ_E_SHAPE: nseq outside 1 .. 16, a segment with rows <= 0, start < 0, start + rows > t_max, slot < 0 or rows outside [0, total_rows); two
 * segments whose row ranges overlap; two segments with the same slot (one would read cache rows the other writes in the same launch: feed a
 * sequence's chunks in consecutive calls); slot_stride < t_max heads 128; ldq / ldo below the row width. */
#define GPTQ_PROMPT_ATTN_MAX_SEQS 16
typedef struct { int32_t row0, rows, start, slot; } gptq_prompt_seg_t;
int gptq_prompt_attn_batch_f16(const void *qkv, int64_t ldq, int total_rows, const gptq_prompt_seg_t *segs, int nseq, void *k_cache,
                               void *v_cache, int64_t slot_stride, void *out, int64_t ldo, void *workspace, size_t workspace_bytes, int heads,
                               int head_dim, int t_max, float base, float scale, const float *rope_table, gptq_stream_t stream);
/* ("fp8 KV cache" above: the rows such a call appended to an fp16 staging cache, converted into the fp8 cache) */
int gptq_kv8_store_f16(const void *k16, const void *v16, int64_t slot_stride, const gptq_prompt_seg_t *segs, int nseq, void *k8, void *v8,
                       void *kexp, void *vexp, int heads, int head_dim, int t_max, gptq_stream_t stream);

/* ---- speculative decoding: attention of a CHUNK of a decoding sequence with the position in device memory (csrc/chunk_attn.hip) ----------------
 * Replaces what HF generate's one-token loop (llama_inference.py:109-115) does R times between qkv_proj and o_proj: `rows` (1 .. 16, a host value: it
 * shapes the grid) consecutive tokens of ONE sequence -- the last accepted token and its drafts -- sit at positions p .. p + rows - 1 with
 * p = *position read on the DEVICE, so a captured graph replays the call at any position.  qkv [rows][3 heads 128] (q | k | v, rows ldq apart) is
 * left untouched; k_cache / v_cache are one slot [t_max][heads 128].  The rotated k and the v of row r go to cache row p + r, bit-identical to what
 * gptq_decode_rope_kv_f16 and gptq_prompt_attn_f16 write for that row and position (rope_table = NULL computes the trig in the kernel, bit-identical
 * to the table of gptq_rope_table_f32); out[r] = softmax(scale q_r . K[0 .. p + r]) V[0 .. p + r], causal inside the chunk, fp32 accumulation on
 * v_mfma_f32_16x16x32_f16, rows ldo apart.  The history [0, p) is streamed ONCE per head for all rows: the key range [0, p + rows) is cut into
 * gptq_decode_attn_chunk_splits(heads, 128, t_max, p + rows) splits of at least 256 tokens (attn_split.h, at most 8 and at most 256 / heads), each
 * a workgroup; one split stores the rows itself (one fp16 rounding), several leave {M, den, fp16 o} records in the workspace and the last to arrive
 * (an arrival ticket, the only atomic) merges them in split order: the same inputs give the same bits on every call.
 * Cache rows at and beyond p + rows are never loaded and, for row r, nothing above p + r reaches the result: stale or NaN rows behind the chunk
 * (rejected drafts) are harmless.  p < 0 marks an idle call: no cache row and no output row is read or written.  A row whose position would be
 * >= t_max is skipped (no cache write, its out row untouched); the rows that fit are served.  No access outside the slot for any *position.
 * Two launches.  The workspace (gptq_decode_attn_chunk_workspace_bytes; 0 for unsupported shapes) is pure scratch: no initialisation, no state
 * between calls -- but two calls that may overlap must not share it.
 * Validated before anything is launched: GPTQ_E_NULL (qkv, position, k_cache, v_cache, out, workspace); GPTQ_E_SHAPE (rows outside 1 .. 16,
 * heads < 1, head_dim != 128, t_max < 1, ldq < 3 heads 128, ldo < heads 128, workspace_bytes too small); GPTQ_E_ALIGN (qkv / caches / workspace /
 * out 16 bytes, position and rope_table 8 bytes, ldq / ldo multiples of 8). */
size_t gptq_decode_attn_chunk_workspace_bytes(int rows, int heads, int head_dim, int t_max);
int gptq_decode_attn_chunk_splits(int heads, int head_dim, int t_max, int len);   /* active splits of a call with p + rows = len */
int gptq_decode_attn_chunk_f16(const void *qkv, int64_t ldq, int rows, const int64_t *position, void *k_cache, void *v_cache, void *out, int64_t ldo,
                               void *workspace, size_t workspace_bytes, int heads, int head_dim, int t_max, float base, float scale,
                               const float *rope_table, gptq_stream_t stream);

/* The same for `seqs` (1 .. 16) decoding SEQUENCES at once, `rows` (1 .. 16) consecutive tokens each, seqs rows <= 128 -- the verify step of batched
 * speculative decoding -- still in TWO launches for any seqs (the sequence is a grid dimension of both kernels).  Both counts are host values: they
 * shape the grid.  Row r of sequence b is qkv + (b rows + r) ldq, its output row out + (b rows + r) ldo; cache slot b is k_cache / v_cache +
 * b slot_stride elements ([t_max][heads 128] each; slot_stride >= t_max heads 128 and a multiple of 8: the engine's [batch][t_max][hidden] layer
 * slice has slot_stride = t_max hidden); positions[b] is read on the DEVICE, so a captured graph replays the call at any positions.
 * Every sequence gets exactly the contract of gptq_decode_attn_chunk_f16 -- RoPE + append at cache rows p_b .. p_b + rows - 1 of its slot, attention
 * causal inside its chunk, its history streamed once per head for all its rows, the same attn_split() cut with the same grid split count, the same
 * record / ticket merge with one ticket per (sequence, head) -- and the same bits: cache rows and output rows are bit-identical to a call of the
 * single-sequence entry on that slot, whatever the other sequences hold.
 * positions[b] < 0 or >= t_max marks an IDLE sequence: nothing of its slot or its output rows is read or written.  A row whose position would be
 * >= t_max is skipped; the rows that fit are served.  No access outside a slot for any position value.
 * The workspace (gptq_decode_attn_chunk_batch_workspace_bytes; 0 for unsupported shapes; for seqs = 1 the size of the single-sequence entry) is pure
 * scratch: no initialisation, no state between calls -- but two calls that may overlap must not share it.
 * Validated before anything is launched: GPTQ_E_NULL (qkv, positions, k_cache, v_cache, out, workspace); GPTQ_E_SHAPE (seqs or rows outside
 * 1 .. 16, seqs rows > 128, heads < 1, head_dim != 128, t_max < 1, ldq < 3 heads 128, ldo < heads 128, slot_stride < t_max heads 128,
 * workspace_bytes too small); GPTQ_E_ALIGN (qkv / caches / workspace / out 16 bytes, positions and rope_table 8 bytes, ldq / ldo / slot_stride
 * multiples of 8). */
size_t gptq_decode_attn_chunk_batch_workspace_bytes(int seqs, int rows, int heads, int head_dim, int t_max);
int gptq_decode_attn_chunk_batch_f16(const void *qkv, int64_t ldq, int seqs, int rows, const int64_t *positions, void *k_cache, void *v_cache,
                                     int64_t slot_stride, void *out, int64_t ldo, void *workspace, size_t workspace_bytes, int heads, int head_dim,
                                     int t_max, float base, float scale, const float *rope_table, gptq_stream_t stream);

/* ---- scoring: the LM head of MANY rows with the cross-entropy inside (reference llama.py:241-258: lm_head over all rows of a segment, shifted
 * labels, CrossEntropyLoss) -- the [M, N] logits never exist in memory.
 *   x [M, K] (ldx)       fp16, the already normalised hidden rows
 *   weight [N, K] (ldw)  fp16, k contiguous: lm_head.weight as stored; bias fp16 [N] or NULL
 *   targets [M]          device int64; a negative target marks an ignored row
 *   nll [M]              out, fp32; lse / argmax [M]: optional outputs (either may be NULL)
 * The logit of column n is z_n = fp16(acc_n), with a bias fp16(fp16(acc_n) + bias_n), acc in fp32 on v_mfma_f32_16x16x32_f16: the bits the tile GEMM
 * would have stored, so the results are the fp32 cross-entropy of the fp16 logits.  lse = max z + log sum exp(z - max); nll = lse - z_target;
 * argmax = the lowest index among the maximal z.  target < 0: nll = 0 (lse and argmax are still written); target >= N: nll = NaN, nothing is read
 * out of bounds.  Any N >= 1 (columns >= N are masked one by one).  Two launches, no atomics: bit-identical from run to run, and a row's results do
 * not depend on M or on the row's position.  The workspace (gptq_lm_head_nll_workspace_bytes(M, N): M ceil(N / 256) records of 16 bytes, 16-byte
 * aligned) is pure scratch: no initialisation, no state between launches.
 * Validated before anything is launched: GPTQ_E_NULL (x, weight, targets, nll, workspace), GPTQ_E_SHAPE (M < 0, N <= 0, K <= 0, ldx < K, ldw < K),
 * GPTQ_E_ALIGN (x / weight 16 bytes, ldx / ldw multiples of 8, bias 8 bytes, targets 8 bytes, nll / lse / argmax 4 bytes, workspace 16 bytes),
 * GPTQ_E_WORKSPACE, GPTQ_E_VARIANT (K % 128 != 0: the caller falls back); M == 0 then returns GPTQ_OK. */
size_t gptq_lm_head_nll_workspace_bytes(int M, int N);
int gptq_lm_head_nll_f16(const void *x, int64_t ldx, const void *weight, int64_t ldw, const void *bias, const int64_t *targets, float *nll,
                         float *lse, int32_t *argmax, int M, int N, int K, void *workspace, size_t workspace_bytes, gptq_stream_t stream);

/* ---- sampling: one token per row of fp16 logits (reference llama_inference.py:119-127: do_sample=True, top_p=0.95, temperature=0.8) in ONE
 * launch (csrc/sample.hip), one workgroup per row, no workspace, no atomics on global memory.
 *   logits [rows, vocab] (ld)  fp16, row r at logits + r ld, ld >= vocab; rows need 2-byte alignment only (a [B, 32001] buffer is fine)
 *   u, temperature, top_p      device float [rows]; top_k device int32 [rows]: every row has its own setting, and a captured graph serves any
 *   ids_out                    device int64 [rows]
 * Per row, with l_i the logits and T, k, p, u the row's parameters:
 *   sanitising   T not finite or <= 0: greedy -- the index of the first maximal logit.  k <= 0 or k >= vocab: top-k off.  p NaN or >= 1: top-p
 *                off; p <= 0: only the top class survives.  u is clamped into [0, 1 - 2^-24], NaN becomes 0.
 *   classes      two tokens are tied iff their fp16 logits compare equal (-0 == +0); a class is kept or dropped whole
 *   weights      w_i = exp((l_i - l_max) / T); -inf weighs 0 and is never drawn
 *   top-k        keeps every token whose logit is >= the k-th largest logit: ALL ties stay, so more than k tokens can survive
 *   top-p        on what top-k kept, of mass Z: token i stays iff the mass of the kept tokens with a strictly larger logit is < p Z
 *   draw         W = the mass of the final kept set, c_j its running sum in ascending token id: the first kept id with c_j > u W
 *   non-finite   a row that holds a NaN or +inf: the index of the first such element, nothing else happens
 * The id written is in [0, vocab) whatever the input.  Weights are the accurate fp32 expf of an IEEE division and are summed as integer
 * multiples of 2^-40 (of 2^-(62 - ceil(log2 vocab)) above 2^22 tokens) of the top class's weight: every mass is within vocab 2^-41 of the exact
 * sum of the fp32 weights, and the same inputs give the same id on every call.
 * Validated before the launch: GPTQ_E_NULL (any pointer, reported first), GPTQ_E_SHAPE (rows < 1, vocab < 1, ld < vocab), GPTQ_E_ALIGN (logits 2
 * bytes, u / temperature / top_k / top_p 4 bytes, ids_out 8 bytes). */
int gptq_sample_rows_f16(const void *logits, int64_t ld, int rows, int vocab, const float *u, const float *temperature, const int32_t *top_k,
                         const float *top_p, int64_t *ids_out, gptq_stream_t stream);

/* ---- speculative sampling: the accept / resample rule for one verify step of `rows` = R >= 2 rows in ONE launch (csrc/spec_sample.hip), one
 * workgroup per row.  The emitted tokens are distributed exactly as the target's, whatever the draft.
 *   logits [R, vocab] (ld)           fp16 target logits: row i is the distribution after ids[0 .. i]; 2-byte alignment, ld >= vocab
 *   draft_logits [R - 1, vocab]      fp16 (ld_draft >= vocab): row i is what ids[i + 1] was drawn from.  NULL: every draft is a point mass
 *   ids                              device int64 [R]: ids[0] the last accepted token, ids[1 .. R - 1] the drafts
 *   temperature, top_p, top_k        device float / float / int32 [R], sanitised as gptq_sample_rows_f16 does
 *   u_accept, u_draw                 device float [R], clamped as u there (u_accept[R - 1] is not used)
 *   pos                              device int64 [1], advanced by the launch
 *   out                              device int64 [R + 1]
 *   workspace                        gptq_spec_sample_workspace_bytes(R) bytes, 8-byte aligned: int64 [R + 1].  Word 0 is the arrival ticket: ZERO
 *                                    before the first launch, it puts itself back to zero (a captured graph replays).  Word 1 + i is row i's
 *                                    record, left there for inspection: bit 32 = the row accepted, the low 32 bits = its token (below)
 * Row i, with p the target row's probabilities under the row's setting -- gptq_sample_rows_f16's classes, all ties kept, top-p on what top-k kept
 * -- d = ids[i + 1], and q the same of draft row i under the SAME setting, or one-hot at d without draft logits:
 *   accept    (i < R - 1) iff u_accept[i] q(d) < p(d): a draft outside p's kept set (or outside [0, vocab)) never survives, one with
 *             p(d) >= q(d) always does.  The row's token is d.
 *   reject    the row's token is the first id, ascending, whose running sum of r = max(p - q, 0) exceeds u_draw[i] sum(r); if sum(r) is 0
 *             (impossible in exact arithmetic) the first maximal target logit
 *   bonus     row R - 1 never accepts; its token is gptq_sample_rows_f16's for that row with u = u_draw[R - 1], to the bit
 *   greedy    a greedy row (temperature 0 or not finite) accepts iff d is the first maximal target logit, and that index is its token
 *   non-finite  a target or draft row with a NaN or +inf -- or a draft row of -inf only -- rejects; the token is what gptq_sample_rows_f16 gives
 *             for the target row with u = u_draw[i]
 * Result: a = the number of leading accepting rows among 0 .. R - 2; out = [a, d_0 .. d_{a-1}, t_a, then copies of t_a]; pos[0] += a + 1.  Every
 * id written is in [0, vocab).  The prefix, out and pos are written in the same launch by the workgroup that arrives last.
 * Arithmetic: p and q are the integer masses of gptq_sample_rows_f16 (same kept set, same bits).  A token's mass goes onto a scale common to both
 * rows by the row's factor c_p = 2^S / W_p (one IEEE double division per row): P(x) = floor(m_p(x) c_p + 1/2), one double multiplication per
 * token, S = 40 (62 - ceil(log2 vocab) above 2^22 tokens), Q likewise (2^S for
 * a point mass); the test is u Q(d) < P(d) in doubles, r = max(P - Q, 0) in integers, the draw gptq_sample_rows_f16's on r.  All sums are integer
 * sums: the same inputs give the same bits on every call.
 * Validated before the launch: GPTQ_E_NULL (any pointer but draft_logits, reported first), GPTQ_E_SHAPE (rows < 2, vocab < 1, ld < vocab,
 * ld_draft < vocab with draft logits), GPTQ_E_WORKSPACE, GPTQ_E_ALIGN (logits 2 bytes, float / int32 arrays 4, int64 arrays and workspace 8). */
size_t gptq_spec_sample_workspace_bytes(int rows);
int gptq_spec_sample_rows_f16(const void *logits, int64_t ld, const void *draft_logits, int64_t ld_draft, int rows, int vocab, const int64_t *ids,
                              const float *temperature, const int32_t *top_k, const float *top_p, const float *u_accept, const float *u_draw,
                              int64_t *pos, int64_t *out, void *workspace, size_t workspace_bytes, gptq_stream_t stream);

/* ---- batched speculative sampling: gptq_spec_sample_rows_f16 for `seqs` = B sequences of `rows` = R rows each in ONE launch, grid (R, B): workgroup
 * (i, b) is row i of sequence b.  The same kernel -- gptq_spec_sample_rows_f16 is its B = 1 launch without the idle rule -- so per sequence the
 * records, out and pos are bit-identical to that entry on the sequence's rows, whatever the neighbours hold and whether they idle.
 *   logits [B R, vocab] (ld)         packed [B, R]: row b R + i is row i of sequence b.  So are ids, temperature, top_k, top_p, u_accept, u_draw
 *   draft_logits [B (R - 1), vocab]  row b (R - 1) + i is draft row i of sequence b (ld_draft).  NULL: every draft is a point mass
 *   pos                              device int64 [B]; pos[b] += a_b + 1 for an active sequence
 *   t_max                            sequence b is ACTIVE iff 0 <= pos[b] < t_max (the rule of gptq_decode_attn_chunk_batch_f16).  The workgroups
 *                                    of an idle sequence read no logits and take no ticket: out[b], pos[b] and the sequence's workspace words stay
 *                                    as they are.  Every workgroup reads pos[b] once, before its ticket; the last arriver writes it behind the last
 *                                    ticket, so all R workgroups of a sequence reach the same verdict
 *   out                              device int64 [B, R + 1]: row b = [a_b, d_0 .. d_{a_b - 1}, t_a, copies of t_a]
 *   workspace                        gptq_spec_sample_batch_workspace_bytes(B, R) = B gptq_spec_sample_workspace_bytes(R) bytes, 8-byte aligned:
 *                                    int64 [B, R + 1], sequence b's words = [its ticket, its R records] (B = 1: the layout above).  Every ticket
 *                                    ZERO before the first launch; each puts itself back
 * No atomics beyond the one ticket per sequence (and the LDS atomics of the select); all sums are integer sums.
 * Validated before the launch: GPTQ_E_NULL (any pointer but draft_logits, reported first), GPTQ_E_SHAPE (seqs < 1, seqs > 65535, rows < 2,
 * vocab < 1, ld < vocab, ld_draft < vocab with draft logits, t_max < 1), GPTQ_E_WORKSPACE, GPTQ_E_ALIGN (as gptq_spec_sample_rows_f16). */
size_t gptq_spec_sample_batch_workspace_bytes(int seqs, int rows);
int gptq_spec_sample_batch_f16(const void *logits, int64_t ld, const void *draft_logits, int64_t ld_draft, int seqs, int rows, int vocab,
                               const int64_t *ids, const float *temperature, const int32_t *top_k, const float *top_p, const float *u_accept,
                               const float *u_draw, int64_t *pos, int64_t t_max, int64_t *out, void *workspace, size_t workspace_bytes,
                               gptq_stream_t stream);

/* ---- logit processors: repetition / presence penalty, logit bias and the min-new-tokens EOS mask, applied IN PLACE to rows of fp16 logits ahead
 * of the sampler, in ONE launch (csrc/logits_process.hip), grid (R, B): workgroup (i, b) edits row b R + i under sequence b's settings and token
 * history.  Every per-sequence setting is in device memory: a captured graph serves any setting.  No workspace, no global atomics: the same inputs
 * give the same bits on every call.
 *   logits [B R, vocab] (ld)     fp16, in place; 2-byte alignment only (ld = 32001 is fine), ld >= vocab
 *   hist [B, ld_hist]            device int32: hist[b, p] = the token sequence b consumed at position p; t_hist <= ld_hist positions can be held
 *   last                         device int64 [B R] or NULL: the tokens consumed by THIS step
 *   len, len_add                 device int64 [B] and a scalar: n_b = len[b] + len_add.  The history of row (i, b) is hist[b, 0 : n_b] followed by
 *                                last[b R + 0 .. i]; without `last` it is hist[b, 0 : n_b + i].  n = its length
 *   gen_start                    device int64 [B]: positions below it are the prompt
 *   repetition_penalty, presence_penalty   device float [B];  min_new_tokens device int32 [B]
 *   eos_ids, n_eos               device int32 [n_eos], 0 <= n_eos <= GPTQ_LOGITS_PROCESS_MAX_EOS, shared by all sequences
 *   bias_ids, bias_vals, n_bias  device int32 / float [n_bias], 0 <= n_bias <= GPTQ_LOGITS_PROCESS_MAX_BIAS, shared by all sequences; the ids
 *                                must be DISTINCT (the caller's duty)
 * Append: with `last`, workgroup (i, b) also writes hist[b, n_b + i] = (int32) last[b R + i]; its siblings read those tokens from `last`, never from
 * hist, so no workgroup reads a hist word another one writes in the same launch.
 * Idle: a row with n_b < 0 or n > t_hist is left untouched and writes nothing (finished rows of a batch, an exhausted cache).
 * One row: S = the ids of its history that lie in [0, vocab) (others are ignored), G = those of S found at a position >= gen_start[b].
 *   sanitising   repetition_penalty not finite or <= 0: 1 (off).  presence_penalty NaN: 0.  min_new_tokens <= 0: off.
 *   1 penalties  every v in S, in fp32 from the fp16 logit l, rounded to fp16 ONCE (nearest even): x = l < 0 ? l rp : l / rp (an IEEE division; -0 is
 *                not < 0 -- the arithmetic of HF's RepetitionPenaltyLogitsProcessor), and for v in G: x -= presence_penalty
 *   2 bias       every listed id in [0, vocab): l = fp16(float(l) + bias), on what step 1 stored (a second rounding).  -inf bans the token
 *   3 EOS mask   if n - gen_start[b] < min_new_tokens[b]: every eos_ids[j] in [0, vocab) becomes fp16 -inf (HF's MinNewTokensLengthLogitsProcessor)
 * NaN and +-inf follow IEEE through these operations.  Nothing else of the row is written.
 * Validated before the launch: GPTQ_E_NULL first (any pointer but `last`, and but eos_ids / bias_ids / bias_vals when their count is not
 * positive), GPTQ_E_SHAPE (B < 1, B > 65535, R < 1, R > GPTQ_LOGITS_PROCESS_MAX_ROWS, vocab < 1, vocab > GPTQ_LOGITS_PROCESS_MAX_VOCAB -- the two
 * bitmaps are 32 KiB of LDS there --, ld < vocab, t_hist < 1, ld_hist < t_hist, n_eos or n_bias outside their range), GPTQ_E_ALIGN (logits 2 bytes,
 * int32 / float arrays 4, int64 arrays 8). */
#define GPTQ_LOGITS_PROCESS_MAX_ROWS 16
#define GPTQ_LOGITS_PROCESS_MAX_EOS 8
#define GPTQ_LOGITS_PROCESS_MAX_BIAS 256
#define GPTQ_LOGITS_PROCESS_MAX_VOCAB 131072
int gptq_logits_process_f16(void *logits, int64_t ld, int seqs, int rows, int vocab, int32_t *hist, int64_t ld_hist, int64_t t_hist,
                            const int64_t *last, const int64_t *len, int64_t len_add, const int64_t *gen_start, const float *repetition_penalty,
                            const float *presence_penalty, const int32_t *min_new_tokens, const int32_t *eos_ids, int n_eos,
                            const int32_t *bias_ids, const float *bias_vals, int n_bias, gptq_stream_t stream);

/* ---- constrained decoding: a deterministic automaton over TOKENS in device memory, one state word per sequence, and ONE launch per step
 * (csrc/constrain.hip), grid (B), one workgroup per sequence b, that advances state[b] by the token the step consumed and sets the logits of every
 * token the NEW state does not allow to fp16 -inf (0xFC00), IN PLACE, ahead of the draw.  Every table is in device memory at a fixed address: a
 * captured graph serves any automaton.  No arithmetic, no atomics, no workspace: the same inputs give the same bits on every call.
 * (tests/constrain_ref.py restates the rules in numpy; quant/constrain.py builds the tables.)
 *   logits [B, vocab] (ld)        fp16, in place; 2-byte alignment only, ld >= vocab; elements vocab .. ld - 1 of a row are never touched.  Rows
 *                                 whose base is 16-byte aligned -- together with their class map's row -- are swept with 16-byte accesses
 *   next [n_states, n_classes]    device int16 (ld_next >= n_classes): next[s][c] = the state behind a token of class c in state s; an entry
 *                                 outside [0, n_states) -- -1 by convention -- says the token is not allowed
 *   cls [n_maps, vocab]           device int16 (ld_cls >= vocab): class maps; cls[m][v] = the class of token v; a class outside [0, n_classes)
 *                                 says the token is never allowed
 *   map_of                        device int32 [B]: the class map of sequence b
 *   state                         device int32 [B], read AND written: >= 0 a state, -1 the row is unconstrained, -2 the row has LEFT its automaton
 *   last                          device int64 [B] or NULL: the tokens consumed by THIS step
 *   len, len_add, t_limit         device int64 [B] and two scalars: n_b = len[b] + len_add
 * The rules of row b, in order:
 *   1 idle         n_b < 0 or n_b > t_limit: nothing is written, and neither the logits nor the tables are read (finished rows of a batch, an
 *                  exhausted cache: the rule of the logit processors)
 *   2 switched off s = state[b] < 0: nothing is written, the row keeps its bits
 *   3 advance      with `last`: s' = next[s][cls[map_of[b]][last[b]]]
 *   4 left         s' = -2 when last[b] lies outside [0, vocab), its class outside [0, n_classes), or the entry outside [0, n_states); also --
 *                  with or without `last` -- when s >= n_states or map_of[b] lies outside [0, n_maps).  state[b] = -2 is stored and the row's
 *                  logits are left untouched: garbage in the tables, or a garbage token, never causes an out-of-range read
 *   5 no token     without `last`: s' = s, and state[b] is not written
 *   6 publish      with `last`: state[b] = s'
 *   7 mask         every v in [0, vocab) whose class lies outside [0, n_classes), or whose entry next[s'][class] lies outside [0, n_states),
 *                  becomes 0xFC00; every other element keeps its bits exactly (NaN, +-inf and -0.0 included)
 * One workgroup per sequence because it reads and writes state[b]: no second workgroup may read the word this one stores.
 * Validated before the launch: GPTQ_E_NULL first (any pointer but `last`), GPTQ_E_SHAPE (B < 1, B > GPTQ_CONSTRAIN_MAX_SEQS, vocab < 1,
 * ld < vocab, n_states outside 1 .. GPTQ_CONSTRAIN_MAX_STATES, n_classes outside 1 .. GPTQ_CONSTRAIN_MAX_CLASSES -- the staged row is 32 KiB of
 * LDS there --, ld_next < n_classes, ld_cls < vocab, n_maps < 1), GPTQ_E_ALIGN (logits and the int16 tables 2 bytes, int32 arrays 4, int64
 * arrays 8). */
#define GPTQ_CONSTRAIN_MAX_SEQS 65535
#define GPTQ_CONSTRAIN_MAX_STATES 32767
#define GPTQ_CONSTRAIN_MAX_CLASSES 16384
int gptq_constrain_rows_f16(void *logits, int64_t ld, int seqs, int vocab, const int16_t *next, int64_t ld_next, int n_states, int n_classes,
                            const int16_t *cls, int64_t ld_cls, int n_maps, const int32_t *map_of, int32_t *state, const int64_t *last,
                            const int64_t *len, int64_t len_add, int64_t t_limit, gptq_stream_t stream);

/* ---- beam search: one step of HF's `_beam_search` (one prompt, do_sample=False, at most one EOS id, no logit processors) on N = `beams` rows
 * of fp16 logits, every piece of bookkeeping in ONE device block, and the in-place move of K/V histories between cache rows (csrc/beam.hip;
 * tests/beam_ref.py restates the rule in float64).
 *
 * The state block: gptq_beam_state_bytes(beams, t_max) bytes, 16-byte aligned, 4-byte words (0 for beams outside 2 .. 16 or t_max < 1).  The
 * HOST writes words 0 .. 9, the scores and the pool before the first step; the select entry trusts t_cap and must be given the block it was
 * sized for.  Per-beam arrays have 16 slots whatever N is.  DEAD = -1e9.
 *   word 0 eos (int32, -1: none)   1 max_new   2 length_penalty (float)   3 early_stopping (0 False, 1 True, 2 "never")
 *        4 t_cap = the t_max the block was sized with   5 beams = N   6 t = steps done   7 open   8 done   9 status   10 .. 15 reserved (0)
 *   16   score[16]   float: the running beams; [0, DEAD, ..] before the first step
 *   32   parent[16]  int32: the last step's parents -- what gptq_kv_reorder_f16 reads
 *   48   token[16]   int64: the last step's tokens -- the next step's input ids
 *   80   pool[16]    5 words each {score float, finished, step, parent, token}: the finished hypotheses in descending score order; an entry
 *                    stands for token at step `step` behind running beam `parent` of step `step` - 1; {DEAD, 0, 0, 0, 0} before the first step
 *   160  cand[32]    4 words each {score float, parent, token, hit}: the 2N candidates of the last step in rank order, for inspection
 *   288  rec[16]     68 words each: launch A's record of a row {max float, log sum float, bad, 0, 2N x (id, fp16 bits)} in (logit descending,
 *                    id ascending) order -- the hand-off between the two launches
 *   1376 parent_at[t_cap][N] int32, then token_at[t_cap][N] int32: the back-pointers; the host rebuilds a hypothesis from them (no token history
 *                    moves on the device): tokens[step] = token, beam = parent, then for u = step - 1 .. 0: tokens[u] = token_at[u][beam],
 *                    beam = parent_at[u][beam]
 * status: bit 0 a row held a NaN or +inf or -inf only (all its candidates score DEAD; parents and ids stay in range); bit 1 the block was not set
 * up for the call (beams differs, t outside [0, t_cap)): nothing but status and done is written.  With done set the step changes nothing.
 *
 * gptq_beam_select_f16: one step on logits [N, vocab] (ld >= vocab, rows 2-byte aligned only; row b follows running beam b), two launches:
 *   1  c(b, v) = fp32(score[b] + log_softmax(logits_b)(v)), log_softmax from the row's maximum and the fp32 log of a fixed-tree sum of exp(l - max):
 *      equal logits of a row give bit-equal scores, and the same inputs the same bits on every call
 *   2  the 2N best candidates by (score descending, b ascending, v ascending) -- vocab >= 2N, so the first step takes them all from beam 0
 *   3  hit[r] = v_r == eos or t + 1 >= min(max_new, t_cap).  The next running beams: the candidates ordered by (score with every hit at DEAD,
 *      descending; rank ascending), the first N of them with that score, their parent b_r and token v_r; row t of the tables
 *   4  candidate r is offered to the pool with score c_r / (t + 1)^length_penalty iff hit[r], r < N, open, and not (pool full before this step
 *      and early_stopping 1).  The pool keeps the best N of its entries and the offers; an entry wins a tie against an offer, offers keep rank order
 *   5  t += 1; open &= any_i (score[0] / L^length_penalty > (pool[i] finished ? the pool's minimum score : DEAD)), L = max_new where
 *      early_stopping is 2 and length_penalty > 0, else t
 *   6  done = not (open and not (pool full and early_stopping 1) and not all 2N candidates hit)
 * Validated before any launch: GPTQ_E_NULL (logits, state), GPTQ_E_SHAPE (beams outside 2 .. 16, vocab < 2 beams, ld < vocab), GPTQ_E_ALIGN
 * (logits 2 bytes, state 16).
 *
 * gptq_kv_reorder_f16: caches [layers][rows][t_max][row_elems] fp16 (layer l at + l layer_stride elements, layer_stride >= rows t_max row_elems).
 * Row b of every layer of both caches becomes a copy of row parent[b] at positions [0, len[0]) -- in place, swaps and cycles included: one
 * thread owns a 16-byte column across all rows, loads what it needs and stores only the rows with parent[b] != b.  parent (int32 [rows]) and len
 * (int64 [1], clamped into [0, t_max]) are DEVICE memory: a captured launch serves every step.  Nothing at or past len is read or written; an
 * identity step writes nothing; a parent outside [0, rows) leaves its row alone.  parent = 0 for all rows replicates row 0 (a prompt).
 * Validated before the launch: GPTQ_E_NULL (the caches, parent, len), GPTQ_E_SHAPE (layers < 1, rows outside 1 .. 16, t_max < 1, row_elems < 8 or
 * not a multiple of 8, layer_stride too small or not a multiple of 8), GPTQ_E_ALIGN (caches 16 bytes, parent 4, len 8). */
#define GPTQ_BEAM_MAX_BEAMS 16
size_t gptq_beam_state_bytes(int beams, int t_max);
int gptq_beam_select_f16(const void *logits, int64_t ld, int beams, int vocab, void *state, gptq_stream_t stream);
int gptq_kv_reorder_f16(void *k_cache, void *v_cache, int layers, int rows, int t_max, int row_elems, int64_t layer_stride, const int32_t *parent,
                        const int64_t *len, gptq_stream_t stream);

/* ---- token log-probabilities: how probable the chosen token of a row of fp16 logits was, where it ranks, and the row's first `top` tokens
 * (csrc/logprobs.hip; tests/logprobs_ref.py restates the rule in float64).  ONE launch, one workgroup per row, rows = 1 .. 128, no workspace.
 *
 * For row r of logits [rows, vocab] (ld >= vocab, rows 2-byte aligned only) and its token ids[r] (int64):
 *   m      = the row's maximum;  S = sum_v expf(fp32(l_v) - m) in fp32, in a fixed order (the tree of gptq_beam_select_f16);
 *   lp(v)  = (fp32(l_v) - m) - logf(S)
 *   order  : tokens by the 16-bit order-preserving key of their fp16 bits, descending (-0 counts as +0), then by id ascending
 *   top_ids / top_logprobs [0 .. top) = the first `top` tokens of that order and their lp;  rank = the 0-based place of ids[r] in that order;
 *   chosen = lp(ids[r]).  Hence rank < top <=> top_ids[rank] == ids[r], and then top_logprobs[rank] has the bits of chosen.
 * top = 0 .. GPTQ_LOGPROBS_MAX_TOP; 0 gives chosen and rank only (top_ids and top_logprobs may be NULL).  vocab >= max(top, 1).
 * -inf entries are legal (a banned token): their lp is -inf and they sort last, in id order among themselves.  A row that holds a NaN or +inf,
 * or -inf only, has no distribution: chosen = NaN, rank = -1, top_ids = 0 .. top - 1, top_logprobs = NaN; the other rows are unaffected.
 * ids[r] outside [0, vocab) gives chosen = NaN and rank = -1; the row's top list is still written.
 * Addressing: chosen and rank are [steps][rows], top_ids and top_logprobs [steps][rows][top].  step == NULL writes slot 0; otherwise the launch
 * reads step[0] on the DEVICE -- a captured launch serves every step of a generation -- and a value outside [0, steps) writes nothing at all.
 * Deterministic: no global atomics, only integer counts go through LDS atomics; the same bits on every call, and a row's record depends neither
 * on the other rows of the launch nor on the slot it goes to.
 * Validated before the launch: GPTQ_E_NULL (logits, ids, chosen, rank; top_ids and top_logprobs when top > 0), GPTQ_E_SHAPE (rows outside
 * 1 .. 128, top outside 0 .. 32, vocab < max(top, 1), ld < vocab, steps < 1), GPTQ_E_ALIGN (logits 2 bytes, ids and step 8, the outputs 4). */
#define GPTQ_LOGPROBS_MAX_TOP 32
int gptq_logprobs_rows_f16(const void *logits, int64_t ld, int rows, int vocab, const int64_t *ids, int top, const int64_t *step, int64_t steps,
                           float *chosen, int32_t *rank, int32_t *top_ids, float *top_logprobs, gptq_stream_t stream);

/* ---- GPTQ solver (the caller that PRODUCES the weights; reference gptq.py:128-228) -------------------------------
 * One column block [i1, i1 + count), count <= 128, of the sequential quantise / error-feedback loop (gptq.py:177-199)
 * for all rows at once, in the reference's own fp32 arithmetic (IEEE division, round-half-even, no contraction).
 *   W [rows, cols] (ldw)    current weights, read only (the block's columns; as the reference, the in-block updates
 *                           live in registers -- its W1 clone -- and W itself changes only through the trailing update)
 *   Hinv [cols, cols] (ldh) upper Cholesky factor of the inverse damped Hessian (gptq.py:160-163)
 *   scale, zero [rows, ldg] grid of row r, group g = column / groupsize (pass groupsize = cols for "no groups");
 *                           the host fits them from W before the block (gptq.py:181-183 -> quantizer.py:32-76)
 *   Q [rows, cols] (ldq)    out: quantised (de-quantised, fp32) weights of the block's columns
 *   Err [rows, count] (lde) out: Err1, for the trailing update W[:, i2:] -= Err1 . Hinv[i1:i2, i2:] (gptq.py:204)
 *   loss_rows [rows]        in/out: += sum over the block's columns of (w - q)^2 / d^2 / 2 (gptq.py:194,202) */
int gptq_solver_block_f32(const float *W, int64_t ldw, const float *Hinv, int64_t ldh, int rows, int cols, int i1, int count,
                          int groupsize, int maxq, const float *scale, const float *zero, int64_t ldg, float *Q, int64_t ldq,
                          float *Err, int64_t lde, float *loss_rows, gptq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GPTQ_MI355X_H */
