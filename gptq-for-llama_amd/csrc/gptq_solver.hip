// gptq_solver.hip -- the sequential inner loop of the GPTQ solver (reference gptq.py:177-199) for one block of
// columns, all rows in parallel.  This is the CALLER side of the hot path: it produces the integer weights that
// QuantLinear.pack (quant_linear.py:325-371) packs and the matvec kernels read.
//
// The reference walks the <= 128 columns of a block one by one with a handful of torch launches per column
// (quantise, loss, outer product, subtract: gptq.py:190-198), i.e. ~1000 dependent launches per block.  Rows never
// interact, so here ONE launch per block gives every weight row to a wave: lane l keeps columns l and l + 64 of the
// block in registers, column i is broadcast with a lane read, rounded to its grid, and the error is fed forward
// into the lanes' remaining columns with the row i of the block's inverse-Hessian factor.  The arithmetic is the
// reference's, operation by operation (IEEE fp32, round-half-even, separate multiply and subtract -- this file is
// compiled without fast-math and without contraction):
//     q    = scale * (clamp(rint(w / scale) + zero, 0, maxq) - zero)         quantizer.py:28-32
//     loss = (w - q)^2 / d^2 ; err = (w - q) / d                              gptq.py:193-195
//     w[j] = w[j] - err * Hinv1[i][j]   for j >= i                            gptq.py:196
// The grid of a column is looked up in per-group (scale, zero) arrays that the host fills before the block from the
// global W, exactly as the reference fits it (gptq.py:181-183 reads W, not the in-block clone W1).
// Outputs: Q (block columns), Err1 (for the trailing update W[:, i2:] -= Err1 . Hinv[i1:i2, i2:], a GEMM the host
// issues, gptq.py:204) and the per-row loss sum (gptq.py:194, :202).
#include "gptq_device.h"
#include "gptq_internal.h"

namespace gptq {

// The column loop of one block for ONE weight row, by one wave: lane l owns columns l and l + 64 of the block.  wrow / hrow point at the block's
// first column of the row / at Hinv[i1][i1]; srow / zrow are the row's grids.  Leaves q (dequantised), e (Err1) and the block's loss sum.
// Both kernels below call it: there is one copy of the arithmetic.
__device__ __forceinline__ void gptq_block_columns(const float *wrow, const float *hrow, int64_t ldh, int i1, int count, int groupsize, float maxq,
                                                   const float *srow, const float *zrow, int lane, float (&q)[2], float (&e)[2], float &loss) {
    float w[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int j = lane + 64 * s;
        w[s] = j < count ? wrow[j] : 0.f;
        q[s] = 0.f;
        e[s] = 0.f;
    }
    loss = 0.f;
    // row i of the factor for this lane's two columns, requested one step ahead
    float h[2];
#pragma unroll
    for (int s = 0; s < 2; s++) h[s] = (lane + 64 * s) < count ? hrow[lane + 64 * s] : 0.f;
    int g_cur = -1;
    float sc = 1.f, zp = 0.f;
    for (int i = 0; i < count; i++) {
        float hn[2] = {0.f, 0.f};
        if (i + 1 < count) {
#pragma unroll
            for (int s = 0; s < 2; s++) hn[s] = (lane + 64 * s) < count ? hrow[(size_t)(i + 1) * ldh + lane + 64 * s] : 0.f;
        }
        const int g = (i1 + i) / groupsize;
        if (g != g_cur) {  // wave-uniform
            g_cur = g;
            sc = srow[g];
            zp = zrow[g];
        }
        const float wi = __shfl((i & 64) ? w[1] : w[0], i & 63, 64);
        const float d = __shfl((i & 64) ? h[1] : h[0], i & 63, 64);  // Hinv1[i][i]
        const float lvl = fminf(fmaxf(rintf(wi / sc) + zp, 0.f), maxq);
        const float qi = sc * (lvl - zp);
        const float diff = wi - qi;
        loss += (diff * diff) / (d * d);
        const float err = diff / d;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int j = lane + 64 * s;
            if (j >= i && j < count) {
                const float p = err * h[s];
                w[s] = w[s] - p;
            }
            if (j == i) {
                q[s] = qi;
                e[s] = err;
            }
            h[s] = hn[s];
        }
    }
}

__global__ void __launch_bounds__(256) gptq_block_kernel(const float *__restrict__ W, int64_t ldw, const float *__restrict__ Hinv, int64_t ldh,
                                                         int rows, int i1, int count, int groupsize, float maxq,
                                                         const float *__restrict__ scale, const float *__restrict__ zero, int64_t ldg,
                                                         float *__restrict__ Q, int64_t ldq, float *__restrict__ Err, int64_t lde,
                                                         float *__restrict__ loss_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float q[2], e[2], loss;
    gptq_block_columns(W + (size_t)row * ldw + i1, Hinv + (size_t)i1 * ldh + i1, ldh, i1, count, groupsize, maxq, scale + (size_t)row * ldg,
                       zero + (size_t)row * ldg, lane, q, e, loss);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int j = lane + 64 * s;
        if (j < count) {
            Q[(size_t)row * ldq + i1 + j] = q[s];
            Err[(size_t)row * lde + j] = e[s];
        }
    }
    if (lane == 0) loss_rows[row] += loss * 0.5f;  // Losses1 / 2 (gptq.py:202)
}

// ---------------------------------------------------------------------------------------------------------------------------------
// solver_layer_kernel: the WHOLE layer in one launch.  Weight rows never interact -- the grid fit, the column loop and the trailing update of
// row r read row r of W and the shared Hinv only -- so a workgroup owns SL_RT = 16 rows for the whole layer and walks the 128-column blocks
// from left to right; nothing synchronises across workgroups: no workspace, no atomics, the same bits on every call, and a row's result does
// not depend on where in a tile it sits.  16 waves, wave w owns row w of the tile for the fit and the column loop (four waves a SIMD: the
// hardware interleaves four of the latency-bound dependent chains, as the per-block launch does); all 16 share the trailing update.
//   per block [i1, i2):
//   1. grid fit (fit != 0): for every group that STARTS in the block the wave takes the row minimum / maximum of W[row, c .. min(c + gs, cols))
//      as it stands in global memory now -- behind the trailing updates of all earlier blocks, before this block's column loop, where the
//      reference fits it (gptq.py:181-183); a group that reaches into later blocks reads columns this workgroup has kept up to date -- and
//      applies quantizer.py's min/max rule (mse = False) operation by operation.  (scale, zero) go to the caller's arrays; one barrier.
//   2. column loop: gptq_block_columns, above.  Q goes to global memory, Err1 to LDS (err[row][k], the A operand of step 3), the loss sum to
//      a register (loss = loss + block * 0.5, block by block, stored once).
//   3. trailing update W[tile, i2:] -= Err1 . Hinv[i1:i2, i2:] on v_mfma_f32_16x16x4_f32, true fp32 operands.  M = 16 is the whole tile, so a
//      column of Hinv has ONE consumer wave: the update is cut into strips of 32 columns, strip s of the block goes to wave s mod 16, and each
//      wave stages its strip privately: the strip's 128 x 32 panel is requested in chunks of 8 k-rows (one float4 a lane, whole 128-byte lines,
//      a ring of 8 chunks always in flight; every workgroup asks for the same panel at about the same time, L2 serves it), each committed into the wave's own
//      double-buffered k-major LDS image ([n-tile][k][16]: the B operand of a k-step is 64 consecutive words) and multiplied.  No workgroup
//      barrier inside the update; the Err1 operand (32 k-steps) stays in registers for all strips of the block.
//      The tile of W is read and written in place by the workgroup that owns it: one __syncthreads (barrier + workgroup-scope fences)
//      separates a block's update from the next block's reads.
constexpr int SL_RT = 16;                     // rows of a tile = waves of a workgroup
constexpr int SL_B = 128;                     // block edge
constexpr int SL_ELD = SL_B + 4;              // row stride of the Err1 image: the 16 x 4 lanes of an A operand read 2 words a bank
constexpr int SL_SN = 32;                     // columns of a strip: two 16-column MFMA tiles, one 128-byte line a k-row
constexpr int SL_KC = 8;                      // k-rows per commit: one float4 a lane
constexpr int SL_DEPTH = 8;                   // chunks of a strip requested ahead of the one being multiplied
constexpr int SL_TS = SL_KC * 16 + 16;        // floats between the two n-tiles of a staged chunk
constexpr int SL_BUF = 2 * SL_TS;             // floats of one staged chunk

__global__ void __launch_bounds__(SL_RT * 64) solver_layer_kernel(float *W, int64_t ldw, const float *__restrict__ Hinv, int64_t ldh, int rows, int cols,
                                                                  int groupsize, float maxq, int sym, int fit, float *scale, float *zero, int64_t ldg,
                                                                  float *__restrict__ Q, int64_t ldq, float *__restrict__ loss_rows) {
    __shared__ __attribute__((aligned(16))) float err[SL_RT * SL_ELD];
    __shared__ __attribute__((aligned(16))) float stage[SL_RT][2][SL_BUF];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * SL_RT, row = row0 + wave;
    const bool live = row < rows;             // (wave-uniform) a wave past the last row fits and solves nothing but shares barriers and strips
    float *const wrow = W + (live ? row : 0) * ldw;
    float *const srow = scale + (live ? row : 0) * ldg, *const zrow = zero + (live ? row : 0) * ldg;
    float total = 0.f;

    for (int i1 = 0; i1 < cols; i1 += SL_B) {
        const int i2 = i1 + SL_B;
        // ---- 1. grids of the groups that start inside this block
        if (fit) {
            if (live) {
                for (int64_t c = ((int64_t)i1 + groupsize - 1) / groupsize * groupsize; c < i2; c += groupsize) {
                    const int len = (int)(c + groupsize < cols ? groupsize : cols - c);
                    float mn = __builtin_inff(), mx = -__builtin_inff();
                    for (int j = lane; j < len; j += 64) {
                        const float v = wrow[c + j];
                        mn = fminf(mn, v);
                        mx = fmaxf(mx, v);
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        mn = fminf(mn, __shfl_xor(mn, o, 64));
                        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                    }
                    float lo = fminf(mn, 0.f), hi = fmaxf(mx, 0.f);                      // quantizer.py find_params, mse = False
                    if (sym) {
                        hi = fmaxf(fabsf(lo), hi);
                        if (lo < 0.f) lo = -hi;
                    }
                    if (lo == 0.f && hi == 0.f) {
                        lo = -1.f;
                        hi = 1.f;
                    }
                    const float sc = (hi - lo) / maxq;
                    const float zp = sym ? (maxq + 1.f) / 2.f : rintf(-lo / sc);
                    if (lane == 0) {
                        srow[c / groupsize] = sc;
                        zrow[c / groupsize] = zp;
                    }
                }
            }
            __syncthreads();                  // the grids are read back by other lanes
        }
        // ---- 2. the column loop of the wave's row
        float q[2] = {0.f, 0.f}, e[2] = {0.f, 0.f}, loss = 0.f;
        if (live) {
            gptq_block_columns(wrow + i1, Hinv + (int64_t)i1 * ldh + i1, ldh, i1, SL_B, groupsize, maxq, srow, zrow, lane, q, e, loss);
            total = total + loss * 0.5f;      // Losses1 / 2 (gptq.py:202)
#pragma unroll
            for (int s = 0; s < 2; s++) Q[row * ldq + i1 + lane + 64 * s] = q[s];
        }
        if (i2 >= cols) break;                // (uniform) the last block has nothing to its right
#pragma unroll
        for (int s = 0; s < 2; s++) err[wave * SL_ELD + lane + 64 * s] = e[s];
        __syncthreads();
        // ---- 3. W[tile, i2:] -= Err1 . Hinv[i1:i2, i2:]
        float a[SL_B / 4];                    // A operand of k-step s: Err1[m = lane & 15][k = 4 s + (lane >> 4)]
#pragma unroll
        for (int s = 0; s < SL_B / 4; s++) a[s] = err[(lane & 15) * SL_ELD + 4 * s + (lane >> 4)];
        const int kr = lane >> 3, c4 = lane & 7;                                          // staging: k-row of a chunk, float4 of the strip
        float *const put = &stage[wave][0][(c4 >> 2) * SL_TS + kr * 16 + 4 * (c4 & 3)];
        const float *const get = &stage[wave][0][lane];
        const int nstrips = (cols - i2) / SL_SN;
        for (int st = wave; st < nstrips; st += SL_RT) {
            const int c0 = i2 + SL_SN * st;
            const float *const src = Hinv + ((int64_t)i1 + kr) * ldh + c0 + 4 * c4;
            float4_t r[SL_DEPTH];                                                         // a ring: SL_DEPTH chunks are always in flight
#pragma unroll
            for (int c = 0; c < SL_DEPTH; c++) r[c] = *(const float4_t *)(src + (int64_t)(SL_KC * c) * ldh);
            float4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int c = 0; c < SL_B / SL_KC; c++) {
                *(float4_t *)(put + (c & 1) * SL_BUF) = r[c % SL_DEPTH];
                if (c + SL_DEPTH < SL_B / SL_KC) r[c % SL_DEPTH] = *(const float4_t *)(src + (int64_t)(SL_KC * (c + SL_DEPTH)) * ldh);
                __builtin_amdgcn_wave_barrier();                                          // the image is the wave's own: LDS serves a wave in order
#pragma unroll
                for (int s = 0; s < SL_KC / 4; s++)
#pragma unroll
                    for (int t = 0; t < 2; t++)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(SL_KC / 4) * c + s], get[(c & 1) * SL_BUF + t * SL_TS + 64 * s], acc[t], 0, 0, 0);
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int m = 0; m < 4; m++) {                                             // D[4 (lane >> 4) + m][lane & 15]
                    const int64_t rr = row0 + 4 * (lane >> 4) + m;
                    if (rr < rows) {
                        float *const p = W + rr * ldw + c0 + 16 * t + (lane & 15);
                        *p = *p - acc[t][m];
                    }
                }
        }
        __syncthreads();                      // the next block's fit and column loop read what other waves of the workgroup stored
    }
    if (live && lane == 0) loss_rows[row] = total;
}

int solver_layer_launch(float *W, int64_t ldw, const float *Hinv, int64_t ldh, int rows, int cols, int groupsize, int maxq, int sym, int fit,
                        float *scale, float *zero, int64_t ldg, float *Q, int64_t ldq, float *loss_rows, hipStream_t s) {
    hipLaunchKernelGGL(solver_layer_kernel, dim3((rows + SL_RT - 1) / SL_RT), dim3(SL_RT * 64), 0, s, W, ldw, Hinv, ldh, rows, cols, groupsize,
                       (float)maxq, sym, fit, scale, zero, ldg, Q, ldq, loss_rows);
    return (int)hipGetLastError();
}

int gptq_block_launch(const float *W, int64_t ldw, const float *Hinv, int64_t ldh, int rows, int i1, int count, int groupsize, int maxq,
                      const float *scale, const float *zero, int64_t ldg, float *Q, int64_t ldq, float *Err, int64_t lde, float *loss_rows,
                      hipStream_t s) {
    hipLaunchKernelGGL(gptq_block_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, W, ldw, Hinv, ldh, rows, i1, count, groupsize, (float)maxq, scale,
                       zero, ldg, Q, ldq, Err, lde, loss_rows);
    return (int)hipGetLastError();
}

}  // namespace gptq
