// hinv_factor.hip -- the inverse Hessian factor of the GPTQ solver (reference gptq.py:157-163): U upper triangular with U^T U = A^-1, A the
// damped Hessian, fp32.  The reference takes three dense library factorisations, chol(A), chol_inv, chol(.., upper).  Here A is factored from
// the LAST column backwards, A = R R^T with R upper triangular (the Cholesky factorisation of A with rows and columns reversed), and
// U = R^-1: A^-1 = R^-T R^-1, R^-1 is upper triangular with a positive diagonal, so it IS the factor the three calls produce.  One
// factorisation and one triangular inverse, 2/3 n^3 flops, no dense A^-1.
//
// Blocked on 128 columns, from the last block i = nb - 1 down to 0, the inverse fused into the same sweep.  Per step:
//   1. hinv_diag_kernel, ONE workgroup of 16 waves: A_ii -> R_ii (stored into A) and U_ii = R_ii^-1 (stored into U, +0 below the diagonal).
//      Thread (column c, row group g) keeps the 16 elements (g + 8 q, c) in registers; the 128 x 128 image in LDS carries only what is
//      broadcast.  Cholesky, column j = 127 .. 0: the threads of column j publish it into the image, ONE barrier, every thread reads
//      w = a_cj / a_jj (one IEEE division) and applies a_rc -= a_rj w to its elements above the diagonal left of j.  The scaling by
//      sqrt(a_jj) (IEEE square root, no rsqrt) is done once behind the loop, for all columns in parallel.  Inverse, row k = 127 .. 0 of
//      R U = I: the row group of k publishes its row of the running right-hand side, ONE barrier, every thread takes u_kc = w_kc / r_kk and
//      applies w_rc -= r_rk u_kc.  No index depends on data: a pivot <= 0 or not finite is recorded (1 + its column, into `info` if that is
//      still 0, a plain vector store by one lane), NaN flows through the arithmetic and the kernel ends as always.
//   2. hinv_step_kernel, one launch: row tiles and panel tiles.
//      panel tile k < i:  R[k, i] = A[k, i] U_ii^T in place (128 x 128, K = 128); it also stores the +0 block U[i, k] below the diagonal.
//      row tile j > i:    U[i, j] = -U_ii sum_{k = i+1 .. j} R[i, k] U[k, j].  The sum has K up to n and only nb - 1 - i block columns exist, so a
//                         row tile is 128 x 32 (four per block column, one 32 x 32 accumulator block per wave): four times the workgroups and a
//                         quarter of the dependent MFMA chain of a 128 x 128 tile.  The sum stays in the accumulators, goes to LDS as the
//                         B operand of the second product, and U_ii streams through the A staging.  Longest sums come first in the grid.
//   3. hinv_trail_kernel: A[a, b] -= R[a, i] R[b, i]^T for the tiles a <= b < i (nothing ever reads the lower triangle of A), numbered
//      row-major over the triangle with XCD x owning a contiguous run, as hessian.hip numbers its tiles.
//   Tile products: v_mfma_f32_32x32x2_f32.  Both operands are staged k-major ([k][width + 4] floats: lane l reads element 2 s + (l >> 5), l & 31 of
//   its block, 32 consecutive words) in chunks of 16 k, register-staged and double-buffered: the next chunk is requested before the
//   products of the current one and committed to the other buffer behind them, one barrier per chunk; the last iteration re-requests
//   the last chunk instead of branching.
// Cross-workgroup ordering is the kernel boundary only; every element has one writer per launch and one summation order: no workspace, no
// atomics, the same bits on every call.
#include "gptq_internal.h"

namespace gptq {

constexpr int HF_B = 128;            // block edge
constexpr int HF_KC = 16;            // k per staged chunk
constexpr int HF_LD = HF_B + 4;      // floats per k-row of a staged image (rows stay 16-byte aligned)
constexpr int HF_RN = 32;            // columns of a row tile
constexpr int HF_DLD = HF_B + 1;     // row stride of the diagonal kernel's image: a column walk touches 32 banks

struct HinvArgs {
    float *A, *U;
    int64_t lda, ldu;
    int32_t *info;
    int nb, i;                       // blocks, current block
    int per;                         // trailing tiles per XCD
};

// ---------------------------------------------------------------------------------------------------------------------------------
// 1. the diagonal block
__global__ void __launch_bounds__(1024) hinv_diag_kernel(const HinvArgs p) {
    __shared__ float img[HF_B * HF_DLD];
    __shared__ float prow[2][HF_B];
    const int tid = threadIdx.x, c = tid & 127;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 7);      // wave-uniform: a wave reads img[row][j] as one broadcast
    const int i0 = p.i * HF_B;
    float *const Ab = p.A + (int64_t)i0 * p.lda + i0;
    float *const Ub = p.U + (int64_t)i0 * p.ldu + i0;

    float x[16];
#pragma unroll
    for (int q = 0; q < 16; q++) x[q] = Ab[(int64_t)(g + 8 * q) * p.lda + c];

    // ---- reversed Cholesky without the scaling: column j of the image is a_.j as it stands when column j + 1 .. 127 are eliminated ----
    int bad = 0;
    if (c == HF_B - 1) {
#pragma unroll
        for (int q = 0; q < 16; q++) img[(g + 8 * q) * HF_DLD + c] = x[q];
    }
#pragma unroll 1
    for (int j = HF_B - 1; j >= 0; j--) {
        __syncthreads();
        const float d = img[j * HF_DLD + j];
        if (bad == 0 && !(d > 0.f && d < __builtin_inff())) bad = i0 + j + 1;
        const float w = img[c * HF_DLD + j] / d;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = g + 8 * q;
            if (r < j) {                                          // (wave-uniform) rows at or below j are finished
                const float v = x[q] - img[r * HF_DLD + j] * w;
                x[q] = (r <= c && c < j) ? v : x[q];
            }
        }
        if (c == j - 1) {
#pragma unroll
            for (int q = 0; q < 16; q++) img[(g + 8 * q) * HF_DLD + c] = x[q];
        }
    }
    __syncthreads();
    const float s = __builtin_sqrtf(img[c * HF_DLD + c]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; q++) {                                // R: r_rc = a_rc / sqrt(a_cc) above, sqrt(a_cc) on, 0 below the diagonal
        const int r = g + 8 * q;
        const float v = r < c ? x[q] / s : (r == c ? s : 0.f);
        img[r * HF_DLD + c] = v;
        if (r <= c) Ab[(int64_t)r * p.lda + c] = v;
    }

    // ---- U = R^-1: backward elimination of R U = I, row k = 127 .. 0; x is the running right-hand side ---------------------------------
#pragma unroll
    for (int q = 0; q < 16; q++) x[q] = (g + 8 * q == c) ? 1.f : 0.f;
    if (g == 7) prow[1][c] = x[15];
#pragma unroll
    for (int qq = 15; qq >= 0; qq--) {
#pragma unroll 1
        for (int gg = 7; gg >= 0; gg--) {
            const int k = 8 * qq + gg;
            __syncthreads();
            const float uk = prow[k & 1][c] / img[k * HF_DLD + k];
            if (g == gg) Ub[(int64_t)k * p.ldu + c] = k <= c ? uk : 0.f;   // row k of U_ii is finished: stored by its row group, +0 below
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int r = g + 8 * q;
                if (r < k) x[q] = x[q] - img[r * HF_DLD + k] * uk;   // (wave-uniform) rows above k
            }
            const float next = gg > 0 ? x[qq] : x[qq > 0 ? qq - 1 : 0];   // row k - 1 lives in register qq, or qq - 1 behind a group of 8
            if (k > 0 && g == ((k - 1) & 7)) prow[(k - 1) & 1][c] = next;
        }
    }
    if (tid == 0) {                                               // the first step of the sweep owns the word; later ones keep the first pivot
        if (p.i == p.nb - 1) *p.info = bad;
        else if (bad != 0 && *p.info == 0) *p.info = bad;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the tile product.  A operand: [128][K], k contiguous.  B operand: [BN][K], k contiguous (B_KMAJOR false) or [K][BN], n contiguous (true).
template <int BN> struct HinvTile {
    static constexpr int WM = BN == HF_B ? 64 : 32, WN = BN == HF_B ? 64 : 32;   // a wave's share: 2 x 2 waves of 64 x 64, or 4 x 1 of 32 x 32
    static constexpr int MB = WM / 32, NB = WN / 32;
    static constexpr int LDB = BN + 4;                                           // floats per k-row of the B image
};

struct HinvLds {
    float a[2][HF_KC * HF_LD];
    float b[2][HF_KC * HF_LD];
};

// a [rows = 128][16] chunk of a k-contiguous operand, transposed into the k-major image: 512 float4, two per thread; the 64 lanes of a wave
// hold 64 consecutive rows of one k quad, so the four scalar stores of a quad each cover 64 consecutive words
struct HinvStageT {
    float4_t r[2];
    __device__ void request(const float *src, int64_t ld, int k0, int tid) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int idx = tid + 256 * q, row = idx & 127, kq = idx >> 7;
            r[q] = *(const float4_t *)(src + (int64_t)row * ld + k0 + 4 * kq);
        }
    }
    __device__ void commit(float *dst, int tid) const {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int idx = tid + 256 * q, row = idx & 127, kq = idx >> 7;
#pragma unroll
            for (int e = 0; e < 4; e++) dst[(4 * kq + e) * HF_LD + row] = r[q][e];
        }
    }
};

// a [16][32] chunk of an n-contiguous operand: already k-major, 128 float4, one for each of the first 128 threads
struct HinvStageN {
    float4_t r;
    __device__ void request(const float *src, int64_t ld, int k0, int tid) {
        if (tid < 128) r = *(const float4_t *)(src + (int64_t)(k0 + (tid >> 3)) * ld + 4 * (tid & 7));
    }
    __device__ void commit(float *dst, int tid) const {
        if (tid < 128) *(float4_t *)(dst + (tid >> 3) * HinvTile<HF_RN>::LDB + 4 * (tid & 7)) = r;
    }
};

template <int BN>
__device__ __forceinline__ void hinv_chunk(const float *la, const float *lb, int wm0, int wn0, int lane,
                                           float16_t (&acc)[HinvTile<BN>::MB][HinvTile<BN>::NB]) {
    using T = HinvTile<BN>;
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int s = 0; s < HF_KC / 2; s++) {
        float fa[T::MB], fb[T::NB];
#pragma unroll
        for (int m = 0; m < T::MB; m++) fa[m] = la[(2 * s + hi) * HF_LD + wm0 + 32 * m + l31];
#pragma unroll
        for (int n = 0; n < T::NB; n++) fb[n] = lb[(2 * s + hi) * T::LDB + wn0 + 32 * n + l31];
#pragma unroll
        for (int m = 0; m < T::MB; m++)
#pragma unroll
            for (int n = 0; n < T::NB; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
}

// acc += A B over K (a multiple of 16, >= 16); StageB is HinvStageT (BN = 128) or HinvStageN (BN = 32).  Ends behind a barrier: LDS is free.
template <int BN, typename StageB>
__device__ __forceinline__ void hinv_product(const float *a_src, int64_t lda, const float *b_src, int64_t ldb, int K, HinvLds &lds, int wm0, int wn0,
                                             float16_t (&acc)[HinvTile<BN>::MB][HinvTile<BN>::NB]) {
    const int tid = threadIdx.x, lane = tid & 63;
    HinvStageT sa;
    StageB sb;
    const int nch = K / HF_KC;
    sa.request(a_src, lda, 0, tid);
    sb.request(b_src, ldb, 0, tid);
    sa.commit(lds.a[0], tid);
    sb.commit(lds.b[0], tid);
    __syncthreads();
    for (int ch = 0; ch < nch; ch++) {
        const int nxt = min(ch + 1, nch - 1) * HF_KC;             // the last iteration stages the last chunk again, into the buffer nobody reads
        sa.request(a_src, lda, nxt, tid);
        sb.request(b_src, ldb, nxt, tid);
        hinv_chunk<BN>(lds.a[ch & 1], lds.b[ch & 1], wm0, wn0, lane, acc);
        sa.commit(lds.a[(ch + 1) & 1], tid);
        sb.commit(lds.b[(ch + 1) & 1], tid);
        __syncthreads();
    }
}

template <int MB, int NB>
__device__ __forceinline__ void hinv_zero(float16_t (&acc)[MB][NB]) {
#pragma unroll
    for (int m = 0; m < MB; m++)
#pragma unroll
        for (int n = 0; n < NB; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2. row tiles (first in the grid, longest sum first) and panel tiles of step i
__global__ void __launch_bounds__(256, 2) hinv_step_kernel(const HinvArgs p) {
    __shared__ __attribute__((aligned(16))) HinvLds lds;
    __shared__ __attribute__((aligned(16))) float sum[HF_B * HinvTile<HF_RN>::LDB];   // row tiles: the 128 x 32 sum as the k-major B operand of -U_ii . sum
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = p.i * HF_B;
    const float *const Uii = p.U + (int64_t)i0 * p.ldu + i0;
    const int nrow = (p.nb - 1 - p.i) * (HF_B / HF_RN);
    const int bid = blockIdx.x;

    if (bid < nrow) {                                             // (workgroup-uniform)
        const int j = p.nb - 1 - bid / (HF_B / HF_RN), c0 = j * HF_B + HF_RN * (bid % (HF_B / HF_RN));
        const int wm0 = 32 * wave;
        float16_t acc[1][1];
        hinv_zero(acc);
        // sum_{k = i+1 .. j} R[i, k] U[k, j]: rows i0 .. of A from column i0 + 128 on, rows i0 + 128 .. of U at columns c0 ..
        hinv_product<HF_RN, HinvStageN>(p.A + (int64_t)i0 * p.lda + i0 + HF_B, p.lda, p.U + (int64_t)(i0 + HF_B) * p.ldu + c0, p.ldu, (j - p.i) * HF_B,
                                        lds, wm0, 0, acc);
#pragma unroll
        for (int r = 0; r < 16; r++) sum[(wm0 + (r & 3) + 8 * (r >> 2) + 4 * hi) * HinvTile<HF_RN>::LDB + l31] = acc[0][0][r];
        hinv_zero(acc);
        __syncthreads();
        // U_ii . sum: U_ii streams through the A staging, the B operand is resident
        HinvStageT sa;
        sa.request(Uii, p.ldu, 0, tid);
        sa.commit(lds.a[0], tid);
        __syncthreads();
        for (int ch = 0; ch < HF_B / HF_KC; ch++) {
            sa.request(Uii, p.ldu, min(ch + 1, HF_B / HF_KC - 1) * HF_KC, tid);
            hinv_chunk<HF_RN>(lds.a[ch & 1], sum + ch * HF_KC * HinvTile<HF_RN>::LDB, wm0, 0, lane, acc);
            sa.commit(lds.a[(ch + 1) & 1], tid);
            __syncthreads();
        }
        float *const out = p.U + (int64_t)(i0 + wm0) * p.ldu + c0 + l31;
#pragma unroll
        for (int r = 0; r < 16; r++) out[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * hi) * p.ldu] = 0.f - acc[0][0][r];   // 0 - 0 is +0
        return;
    }

    const int k = bid - nrow, k0 = k * HF_B;                      // panel tile k < i: R[k, i] = A[k, i] U_ii^T
    const int wm0 = 64 * (wave >> 1), wn0 = 64 * (wave & 1);
    float16_t acc[2][2];
    hinv_zero(acc);
    float *const Aki = p.A + (int64_t)k0 * p.lda + i0;
    hinv_product<HF_B, HinvStageT>(Aki, p.lda, Uii, p.ldu, HF_B, lds, wm0, wn0, acc);   // every read of A[k, i] is behind its last barrier
    float *const Uik = p.U + (int64_t)i0 * p.ldu + k0;            // below the diagonal of U: +0
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = wm0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hi, col = wn0 + 32 * n + l31;
                Aki[(int64_t)row * p.lda + col] = acc[m][n][r];
                Uik[(int64_t)row * p.ldu + col] = 0.f;
            }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3. trailing update of step i: A[a, b] -= R[a, i] R[b, i]^T, a <= b < i
__global__ void __launch_bounds__(256, 2) hinv_trail_kernel(const HinvArgs p) {
    __shared__ __attribute__((aligned(16))) HinvLds lds;
    const int nt = p.i;
    const int64_t tile = (int64_t)(blockIdx.x & 7) * p.per + (blockIdx.x >> 3);
    const int64_t ntiles = (int64_t)nt * (nt + 1) / 2;
    if (tile >= ntiles) return;                                   // (workgroup-uniform) padding of the last runs
    // row ta of the triangle starts at S(ta) = ta nt - ta (ta - 1) / 2: an estimate from the square root, then exact integer steps
    const double nh = nt + 0.5;
    int ta = (int)(nh - sqrt(nh * nh - 2.0 * (double)tile));
    ta = max(0, min(ta, nt - 1));
    auto row_start = [&](int r) { return (int64_t)r * nt - (int64_t)r * (r - 1) / 2; };
    while (ta > 0 && row_start(ta) > tile) ta--;
    while (ta + 1 < nt && row_start(ta + 1) <= tile) ta++;
    const int tb = ta + (int)(tile - row_start(ta));

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = 64 * (wave >> 1), wn0 = 64 * (wave & 1);
    const int i0 = p.i * HF_B;
    float16_t acc[2][2];
    hinv_zero(acc);
    hinv_product<HF_B, HinvStageT>(p.A + (int64_t)ta * HF_B * p.lda + i0, p.lda, p.A + (int64_t)tb * HF_B * p.lda + i0, p.lda, HF_B, lds, wm0, wn0, acc);
    float *const out = p.A + (int64_t)ta * HF_B * p.lda + (int64_t)tb * HF_B;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float *const e = out + (int64_t)(wm0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hi) * p.lda + wn0 + 32 * n + l31;
                *e = *e - acc[m][n][r];
            }
}

// n = 128 nb; two or three launches per block step, no host synchronisation; the first launch error ends the sweep
int hinv_factor_launch(float *A, int64_t lda, int n, float *U, int64_t ldu, int32_t *info, hipStream_t s) {
    HinvArgs a{};
    a.A = A;
    a.U = U;
    a.lda = lda;
    a.ldu = ldu;
    a.info = info;
    a.nb = n / HF_B;
    for (int i = a.nb - 1; i >= 0; i--) {
        a.i = i;
        const int64_t ntiles = (int64_t)i * (i + 1) / 2;
        a.per = (int)((ntiles + 7) / 8);
        hipLaunchKernelGGL(hinv_diag_kernel, dim3(1), dim3(1024), 0, s, a);
        const int nstep = (a.nb - 1 - i) * (HF_B / HF_RN) + i;
        if (nstep > 0) hipLaunchKernelGGL(hinv_step_kernel, dim3(nstep), dim3(256), 0, s, a);
        if (i > 0) hipLaunchKernelGGL(hinv_trail_kernel, dim3(8 * a.per), dim3(256), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipGetLastError();
}

}  // namespace gptq
