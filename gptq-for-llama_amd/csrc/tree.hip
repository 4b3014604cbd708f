// tree.hip -- what follows the verify pass of a draft TREE (include/gptq_mi355x.h "tree speculative decoding"; the attention of the tree's nodes is
// the TREE instance of chunk_attn.hip):
//   gptq_tree_accept_greedy    the greedy accept rule walked down the tree, ONE wave, no atomics;
//   gptq_kv_tree_compact_f16   the accepted path's cache rows become a contiguous sequence, every layer, K and V, in place, ONE launch.
//
// The accept.  Lane c < rows holds node c: its token, its parent, the argmax of its logits row.  From n = the root: a ballot over the lanes with
// parent == n and token == best[n] -- the lowest set bit is the lowest-index child the greedy rule agrees with --, n becomes that child; the walk
// ends where the ballot is empty, after a accepted drafts (a <= rows - 1: a child's index is above its parent's, anything else is no child).
// The wave then writes path[0 .. 15] (the node per accepted depth, path[0] = 0; -1 beyond a), the out row in the layout of the chain's verify
// step -- [a, best[path[0]], .., best[path[a]], copies of the last]: the a + 1 tokens a step emits, the accepted drafts and the bonus token --
// and advances the position by a + 1.  Integers in a fixed order: the same inputs give the same bits.
//
// The compaction.  Node path[i] sits in cache row p + path[i], rotated at p + i (its depth); it belongs in row p + i.  One thread owns a 16-byte
// column (layer, k or v, chunk) of the 16 rows p .. p + 15: it loads every row path[i] != i, i <= a, into registers and then stores them to
// rows p + i -- the reorder of beam.hip, so no order between threads matters, and path[i] >= i means no row is read behind its overwrite even
// within a thread that stored as it went.  A chain (path[i] = i) or an empty accept stores nothing.  p, a and the path are read from device
// memory: one captured launch serves every step.  A record that is not one this file's accept writes (a outside 0 .. 15, a path that does not
// ascend from 0, rows outside the cache) moves nothing.
#include "../../include/gptq_mi355x.h"
#include "gptq_internal.h"

namespace {

using gptq::aligned;

constexpr int TR_MAX = 16;                                 // nodes of a tree (the rows of the chunk attention)

__global__ __launch_bounds__(64) void tree_accept_kernel(const int64_t *tok, const int32_t *parent, const int64_t *best, int rows, int64_t *pos,
                                                         int64_t *out, int32_t *path) {
    const int lane = threadIdx.x;
    const bool node = lane >= 1 && lane < rows;
    const int64_t t = node ? tok[lane] : 0;
    const int par = node ? parent[lane] : -1;
    int n = 0, a = 0, mine = lane == 0 ? 0 : -1;           // lane i < 16 ends with path[i]
    int64_t bonus = best[0];
    for (int i = 1; i < TR_MAX; i++) {                     // (uniform: every lane takes part in the ballot)
        const uint64_t hit = __ballot(node && lane > n && par == n && t == bonus);
        if (hit == 0) break;
        n = __builtin_ctzll(hit);
        a = i;
        if (lane == i) mine = n;
        bonus = best[n];
    }
    if (lane < TR_MAX) path[lane] = mine;
    // out[1 + i] = best[path[min(i, a)]]: lane i <= a reads its own node's argmax, the others take the bonus token
    if (lane < rows) out[1 + lane] = lane <= a ? best[mine] : bonus;
    if (lane == 0) {
        out[0] = a;
        pos[0] += a + 1;
    }
}

constexpr int TC_NT = 256;

__global__ __launch_bounds__(TC_NT) void kv_tree_compact_kernel(uint16_t *k_cache, uint16_t *v_cache, int layers, int t_max, int row_elems,
                                                                int64_t layer_stride, const int64_t *pos, const int64_t *accepted,
                                                                const int32_t *path) {
    const int64_t a = accepted[0];
    if (a < 1 || a >= TR_MAX) return;
    const int64_t p = pos[0] - a - 1;                      // the root's row: the position was advanced by a + 1 behind the accept
    if (p < 0 || p >= t_max) return;
    int src[TR_MAX];
    bool ok = true, anymove = false;
#pragma unroll
    for (int i = 1; i < TR_MAX; i++) {
        const int s = i <= a ? path[i] : i;
        ok = ok && s >= i && s < TR_MAX && p + s < t_max && (i == 1 || i > a || s > src[i - 1]);
        src[i] = s;
        anymove |= s != i;
    }
    if (!ok || !anymove) return;
    const int chunks = row_elems >> 3;
    const int64_t columns = (int64_t)chunks * 2 * layers;
    const int64_t i = (int64_t)blockIdx.x * TC_NT + threadIdx.x;
    if (i >= columns) return;
    const int64_t lk = i / chunks, ch = i - lk * chunks;    // a wave reads consecutive 16-byte chunks of a row
    uint16_t *base = ((lk & 1) ? v_cache : k_cache) + (lk >> 1) * layer_stride + p * row_elems + ch * 8;
    u32x4 reg[TR_MAX];
#pragma unroll
    for (int d = 1; d < TR_MAX; d++)
        if (src[d] != d) reg[d] = *(const u32x4 *)(base + (int64_t)src[d] * row_elems);
#pragma unroll
    for (int d = 1; d < TR_MAX; d++)
        if (src[d] != d) *(u32x4 *)(base + (int64_t)d * row_elems) = reg[d];
}

}  // namespace

extern "C" int gptq_tree_accept_greedy(const int64_t *tokens, const int32_t *parent, const int64_t *best, int rows, int64_t *position, int64_t *out,
                                       int32_t *path, gptq_stream_t stream) {
    if (!tokens || !parent || !best || !position || !out || !path) return GPTQ_E_NULL;
    if (rows < 1 || rows > TR_MAX) return GPTQ_E_SHAPE;
    if (!aligned(tokens, 8) || !aligned(parent, 4) || !aligned(best, 8) || !aligned(position, 8) || !aligned(out, 8) || !aligned(path, 4))
        return GPTQ_E_ALIGN;
    hipLaunchKernelGGL(tree_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tokens, parent, best, rows, position, out, path);
    return (int)hipGetLastError();
}

extern "C" int gptq_kv_tree_compact_f16(void *k_cache, void *v_cache, int layers, int t_max, int row_elems, int64_t layer_stride,
                                        const int64_t *position, const int64_t *accepted, const int32_t *path, gptq_stream_t stream) {
    if (!k_cache || !v_cache || !position || !accepted || !path) return GPTQ_E_NULL;
    if (layers < 1 || t_max < 1 || row_elems < 8 || row_elems % 8 != 0 || layer_stride < (int64_t)t_max * row_elems || layer_stride % 8 != 0)
        return GPTQ_E_SHAPE;
    if (!aligned(k_cache, 16) || !aligned(v_cache, 16) || !aligned(position, 8) || !aligned(accepted, 8) || !aligned(path, 4)) return GPTQ_E_ALIGN;
    const int64_t columns = (int64_t)(row_elems >> 3) * 2 * layers;
    hipLaunchKernelGGL(kv_tree_compact_kernel, dim3((unsigned)((columns + TC_NT - 1) / TC_NT)), dim3(TC_NT), 0, (hipStream_t)stream,
                       (uint16_t *)k_cache, (uint16_t *)v_cache, layers, t_max, row_elems, layer_stride, position, accepted, path);
    return (int)hipGetLastError();
}
