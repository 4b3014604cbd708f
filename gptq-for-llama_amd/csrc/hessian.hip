// hessian.hip -- the calibration Hessian of the GPTQ solver (reference gptq.py:71-96): H <- decay H + weight X^T X in place, X fp16 [tokens][k]
// as llama.py's hooks deliver it, H fp32 [k][k].  The reference upcasts X, scales and transposes it into a fresh buffer and runs a full
// K x T x K fp32 GEMM per calibration batch; here the batch is read once as fp16 and only half of the product is computed:
//   * fp16 x fp16 is exact in fp32, so v_mfma_f32_32x32x16_f16 with fp32 accumulation sums the exact products x_i x_j (the reference rounds
//     sqrt(2/n) x to fp32 first); the scale is applied once, to the sum, in the epilogue.
//   * H is symmetric and both operands are column panels of the SAME array: only the 128 x 128 tiles (i <= j) exist.  An off-diagonal tile
//     stages two panels, a diagonal tile stages one and reads it for both operands (and its wave below the diagonal issues no products).
//   * the reduction runs over tokens, the strided dimension of X: a chunk of 64 tokens x 128 columns of a panel is the swizzled 256-byte-row
//     LDS image of attn_device.h, register-staged (the next chunk is requested before the products of the current one and committed behind
//     the barrier that ends it), and the token-major image is read in the MFMA operand layout by ds_read_b64_tr_b16, exactly as prompt_attn.hip
//     reads V.  Both operands use the same permuted token order inside a 16-token step, so the sum is unchanged.
//   * a workgroup is four waves, each owning a 64 x 64 quarter (2 x 2 MFMA blocks, 64 accumulators).  Rows past `tokens` and columns past k
//     are staged as zeros and never stored.
//   * epilogue: v = fma(decay, H_ij, weight acc) on the accumulators, stored at (i, j) as 128-byte row segments, and the same v stored at
//     (j, i) after a transpose through LDS, again as 128-byte row segments.  In a diagonal tile only the elements on and above the diagonal
//     are taken and mirrored, so H[j][i] has the bits of H[i][j] by construction.  Tile (i, j) is the only reader and writer of H(i, j) and
//     H(j, i): in place without any ordering between workgroups, no workspace, no atomics, one fixed summation order -> the same bits on
//     every call.
//   * the tiles are numbered row-major over the triangle and XCD x (workgroup b runs on XCD b % 8) owns a contiguous run of that list, as
//     gemm8's tile order does: the workgroups an XCD runs together share the row panel and walk neighbouring column panels through its L2.
#include "attn_device.h"
#include "gptq_internal.h"

namespace gptq {

constexpr int HS_TILE = 128;   // columns of a panel = edge of an output tile
constexpr int HS_TC = 64;      // tokens per staged chunk

struct HessianArgs {
    const half_t *x;
    float *H;
    int64_t ldx, ldh;
    int tokens, k;
    int nt;               // panels: ceil(k / 128)
    int per;              // tiles per XCD: ceil(nt (nt + 1) / 2 / 8)
    float decay, weight;
};

// two workgroups per CU (2 x 32 KiB of LDS, <= 256 registers per lane): one stages while the other multiplies
__global__ void __launch_bounds__(256, 2) hessian_update_kernel(const HessianArgs a) {
    __shared__ __attribute__((aligned(16))) half_t img[2][HS_TC * HS_TILE];   // panel i, panel j; the epilogue's transpose buffers afterwards

    // ---- which tile: XCD x owns the contiguous run [x per, (x + 1) per) of the row-major list of the triangle -----------------------
    const int64_t tile = (int64_t)(blockIdx.x & 7) * a.per + (blockIdx.x >> 3);
    const int64_t ntiles = (int64_t)a.nt * (a.nt + 1) / 2;
    if (tile >= ntiles) return;                                  // (workgroup-uniform) padding of the last runs
    // row ti starts at S(ti) = ti nt - ti (ti - 1) / 2; an estimate from the square root, then exact integer steps
    const double nh = a.nt + 0.5;
    int ti = (int)(nh - sqrt(nh * nh - 2.0 * (double)tile));
    ti = max(0, min(ti, a.nt - 1));
    auto row_start = [&](int r) { return (int64_t)r * a.nt - (int64_t)r * (r - 1) / 2; };
    while (ti > 0 && row_start(ti) > tile) ti--;
    while (ti + 1 < a.nt && row_start(ti + 1) <= tile) ti++;
    const int tj = ti + (int)(tile - row_start(ti));
    const bool diag = ti == tj;
    const int i0 = ti * HS_TILE, j0 = tj * HS_TILE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;                     // the wave's 64 x 64 quarter: rows 64 wr of panel i, columns 64 wc of panel j
    const int l31 = lane & 31, hi = lane >> 5;
    const bool active = !(diag && wr > wc);                      // (wave-uniform) the quarter below the diagonal is the mirror of the one above

    // ---- staging: 1024 16-byte chunks per panel and token chunk, four per thread (16 lanes = one 256-byte image row) ----------------
    const int srow = tid >> 4, sch = tid & 15;
    const bool ci_ok = i0 + 8 * sch < a.k, cj_ok = !diag && j0 + 8 * sch < a.k;   // k % 8 == 0: a 16-byte chunk is inside or outside
    const half_t *const xi = a.x + i0 + 8 * sch, *const xj = a.x + j0 + 8 * sch;
    u32x4 ireg[4], jreg[4];
    auto request = [&](int t0) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t = t0 + srow + 16 * q;
            ireg[q] = u32x4{0u, 0u, 0u, 0u};
            jreg[q] = u32x4{0u, 0u, 0u, 0u};
            if (t < a.tokens) {
                if (ci_ok) ireg[q] = *(const u32x4 *)(xi + (int64_t)t * a.ldx);
                if (cj_ok) jreg[q] = *(const u32x4 *)(xj + (int64_t)t * a.ldx);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int off = attn_lds_off(srow + 16 * q, sch);
            *(ATTN_LDS u32x4 *)((ATTN_LDS char *)img[0] + off) = ireg[q];
            if (!diag) *(ATTN_LDS u32x4 *)((ATTN_LDS char *)img[1] + off) = jreg[q];
        }
    };

    float16_t acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[u][v][r] = 0.f;

    // transposed read: within a 16-lane group lane (tq, tp) addresses row tq, columns 4 tp .. 4 tp + 3 of a 4 x 16 block and receives column
    // g16 of it.  Operand element e of lane half hi is token 16 s + 8 (e >> 2) + 4 hi + (e & 3) for BOTH operands.
    const int g16 = lane & 15, tq = g16 >> 2, tp = g16 & 3, g1 = (lane >> 4) & 1;
    const half_t *const pa = img[0], *const pb = img[diag ? 0 : 1];
    auto fragment = [&](const half_t *p, int cb, int s) {         // 32 columns 32 cb .. of the panel, tokens 16 s .. of the chunk
        const int r0 = 16 * s + 4 * hi + tq, ch = 4 * cb + 2 * g1 + (tp >> 1);
        const half4_t lo = attn_tr_read(p, attn_lds_off(r0, ch) + 8 * (tp & 1));
        const half4_t up = attn_tr_read(p, attn_lds_off(r0 + 8, ch) + 8 * (tp & 1));
        return half8_t{lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
    };

    const int nchunks = (a.tokens + HS_TC - 1) / HS_TC;
    request(0);
    commit();
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        if (c + 1 < nchunks) request((c + 1) * HS_TC);            // in flight under the products of this chunk
        if (active) {
#pragma unroll
            for (int s = 0; s < HS_TC / 16; s++) {
                half8_t fa[2], fb[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    fa[u] = fragment(pa, 2 * wr + u, s);
                    fb[u] = fragment(pb, 2 * wc + u, s);
                }
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int v = 0; v < 2; v++) acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[u], fb[v], acc[u][v], 0, 0, 0);
            }
        }
        __syncthreads();                                         // every wave is done with the chunk
        if (c + 1 < nchunks) {
            commit();
            __syncthreads();
        }
    }

    // ---- epilogue.  Accumulator r of a block is row (r & 3) + 8 (r >> 2) + 4 hi, column l31.  One 32 x 32 block at a time: update and store
    // at (i, j), leave the values in the wave's transpose buffer [column][row] (33 floats per row), read that by rows and store at (j, i).
    float *const tb = (float *)&img[0][0] + wave * (32 * 33);
    const bool read_h = a.decay != 0.f;                           // decay 0 (the first batch) overwrites: H is not read
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int gi0 = i0 + 64 * wr + 32 * u, gj0 = j0 + 64 * wc + 32 * v;
            const int gj = gj0 + l31;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * hi, gi = gi0 + m;
                const bool ok = gi < a.k && gj < a.k && (!diag || gi <= gj);
                float *const h = a.H + (int64_t)gi * a.ldh + gj;
                const float old = ok && read_h ? *h : 0.f;
                const float val = __builtin_fmaf(a.decay, old, a.weight * acc[u][v][r]);
                if (ok) *h = val;
                tb[l31 * 33 + m] = val;
            }
            __syncthreads();
            const int gi = gi0 + l31;                             // now the lane is the ROW index of the block, the loop its column
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int n = 2 * q + hi, gjr = gj0 + n;
                const float val = tb[n * 33 + l31];
                if (gjr < a.k && gi < a.k && (!diag || gi < gjr)) a.H[(int64_t)gjr * a.ldh + gi] = val;
            }
            __syncthreads();
        }
}

int hessian_update_launch(const half_t *x, int64_t ldx, int tokens, int k, float *H, int64_t ldh, float decay, float weight, hipStream_t s) {
    HessianArgs a{};
    a.x = x;
    a.H = H;
    a.ldx = ldx;
    a.ldh = ldh;
    a.tokens = tokens;
    a.k = k;
    a.nt = (k + HS_TILE - 1) / HS_TILE;
    const int64_t ntiles = (int64_t)a.nt * (a.nt + 1) / 2;
    a.per = (int)((ntiles + 7) / 8);
    a.decay = decay;
    a.weight = weight;
    hipLaunchKernelGGL(hessian_update_kernel, dim3(8 * a.per), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace gptq
