// verify_tree.hip -- the kernels l2z_verify_tree adds to the batched step (host side: verify_host.cpp): the verify pass of
// verify.hip for the nodes of a TREE of guesses.  Node i stands for position pos0 + depth_i; its K / V rows sit in
// PHYSICAL cache row pos0 + i (the G_QKV_ROWS epilogue stores there through a shifted base), and row i attends to the cache
// rows below pos0 and to its own ancestors' rows.
//
// PATH INVARIANCE (include/llama2_hip_test.h): what row i computes equals, bit for bit, what l2z_verify's row depth_i
// computes when the tokens on the path root -> i are given as a chain.  The score buffer is indexed by POSITION (slot
// t - seg0, as verify_device.h's), only the ADDRESS of a tree position's K / V row depends on the row: it is the row's
// ancestor at that depth.  Every order is verify_device.h's: the TPR lanes' partial dot, a wave's max and sum over slots
// lane + 64 j, group g = slot mod G adding its V rows in increasing slot (one fma per row and slot), the groups in g
// order, the segments in segment order.  A position deeper than the row is masked exactly as a later position of a
// chain is: score -inf, weight exactly 0, V row skipped.
#include "batch_decode.h"
#include "kernel_common.h"
#include "verify_device.h"

namespace l2z {
namespace {

constexpr int kVtUB = 2;  // the tree's K rows a lane has in flight beside the context's kVaUB
constexpr int kVvUB = 8;  // the tree's V rows a lane has in flight (those of its own group's slots are loaded)

// Block (h, seg): head h over the positions t of segment seg that the call's rows see, t <= pos0 + max_depth.
// Positions below pos0 are context: one K / V row each, loaded once for all rows (verify_attention_body's loops).
// Position pos0 + d is a tree slot: one K / V row per node of depth d, used by the rows below that node.
__global__ __launch_bounds__(kVaBlock) void verify_tree_attention_kernel(const VerifyTreeAttnArgs a, const int n, const int max_depth)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<kBatchMax>];  // scores [row][slot], then the groups' V sums
    const VerifyTreeTable *tt = a.tree;
    const int h = blockIdx.x, seg = blockIdx.y;
    const int tid = threadIdx.x;
    const int hs = a.head_size, E = hs >> 2;
    int TPR = 1;
    while (TPR < E) TPR <<= 1;
    const int G = kVaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int seg0 = seg * kVerifySeg;
    const int nk = min(seg0 + kVerifySeg, a.pos0 + max_depth + 1) - seg0;  // slots 0 .. nk - 1 are all the call sees here
    const int nctx = min(max(a.pos0 - seg0, 0), nk);                       // slots below nctx are context, the rest tree slots
    const int d0 = max(0, seg0 - a.pos0);                                  // rows shallower than d0 end before this segment
    unsigned act = 0;  // the rows this segment belongs to
    for (int d = d0; d <= max_depth; d++) act |= tt->level[d];
    const size_t head_off = (size_t)(h / a.kv_mul) * a.kv_head_stride;
    const float *kbase = a.kc + head_off, *vbase = a.vc + head_off;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const float div = sqrtf((float)hs);
    v4f qv[kBatchMax];
#pragma unroll
    for (int i = 0; i < kBatchMax; i++)
        qv[i] = ((act >> i) & 1u) && c < E ? *(const v4f *)(a.q + (size_t)i * a.ldq + (size_t)h * hs + 4 * c) : zero;
    // The tree's K rows go a node per group, kVtUB nodes a round: the slot is the node's position, the address its physical
    // row.  The first round is asked for here, before the context loop, so that it arrives behind it.
    v4f tk[kVtUB];
#pragma unroll
    for (int u = 0; u < kVtUB; u++)
        tk[u] = c < E ? *(const v4f *)(kbase + (size_t)(a.pos0 + min(g + G * u, n - 1)) * hs + 4 * c) : zero;  // clamped: dropped below
    // scores sc[i][t - seg0] = q_i . k_t / sqrt(head_size).  Context: every row sees every slot.
    for (int tl0 = g; tl0 < nctx; tl0 += G * kVaUB) {
        v4f kv[kVaUB];
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int t = seg0 + min(tl0 + G * u, nctx - 1);  // clamped: dropped below
            kv[u] = c < E ? *(const v4f *)(kbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int tl = tl0 + G * u;
#pragma unroll
            for (int i = 0; i < kBatchMax; i++)
                if ((act >> i) & 1u) {
                    const float p = lanes_sum(hsum4(fma4(qv[i], kv[u], zero)), TPR);
                    if (c == 0 && tl < nctx) sc[i * kVerifySeg + tl] = p / div;
                }
        }
    }
    // Tree slots: -inf where the slot is deeper than the row ...
    for (int idx = tid; idx < kBatchMax * (nk - nctx); idx += kVaBlock) {
        const int i = idx % kBatchMax, tl = nctx + idx / kBatchMax;
        if (i < n && tt->depth[i] < seg0 + tl - a.pos0) sc[i * kVerifySeg + tl] = -INFINITY;
    }
    // ... and node j's key against the rows below it (j itself included).  (Another element of sc than any the fill above
    // wrote.)  The next round's rows are asked for before this round's dots.
    for (int j0 = g; j0 < n; j0 += G * kVtUB) {
        v4f kv[kVtUB];
        int tl[kVtUB];
        unsigned below[kVtUB];
#pragma unroll
        for (int u = 0; u < kVtUB; u++) {
            const int j = j0 + G * u, jc = min(j, n - 1);
            kv[u] = tk[u];
            tl[u] = a.pos0 + tt->depth[jc] - seg0;
            below[u] = j < n && tl[u] >= 0 && tl[u] < kVerifySeg ? tt->below[jc] & act : 0u;
        }
        if (j0 + G * kVtUB < n) {
#pragma unroll
            for (int u = 0; u < kVtUB; u++)
                tk[u] = c < E ? *(const v4f *)(kbase + (size_t)(a.pos0 + min(j0 + G * (kVtUB + u), n - 1)) * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVtUB; u++) {
#pragma unroll
            for (int i = 0; i < kBatchMax; i++)
                if ((act >> i) & 1u) {
                    const float p = lanes_sum(hsum4(fma4(qv[i], kv[u], zero)), TPR);
                    if (c == 0 && ((below[u] >> i) & 1u)) sc[i * kVerifySeg + tl[u]] = p / div;
                }
        }
    }
    __syncthreads();
    const SegSlots s = verify_slots(a, h, act);  // (the sweep and the fold: where the rows' partials go)
    segment_softmax_sweep<kBatchMax>(s, seg, nk, sc);
    __syncthreads();
    // acc_i = sum over slots of e[i][slot] v: group g takes slots g, g + G, ... in increasing slot -- its context slots ...
    v4f acc[kBatchMax];
#pragma unroll
    for (int i = 0; i < kBatchMax; i++) acc[i] = zero;
    for (int tl0 = g; tl0 < nctx; tl0 += G * kVaUB) {
        v4f vv[kVaUB];
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int t = seg0 + min(tl0 + G * u, nctx - 1);
            vv[u] = c < E ? *(const v4f *)(vbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int tl = tl0 + G * u;
            if (tl < nctx) {
#pragma unroll
                for (int i = 0; i < kBatchMax; i++)
                    if ((act >> i) & 1u) {
                        const float wt = sc[i * kVerifySeg + tl];
                        if (wt > 0.0f) {
                            const v4f w4 = {wt, wt, wt, wt};
                            acc[i] = fma4(w4, vv[u], acc[i]);
                        }
                    }
            }
        }
    }
    // ... then its tree slots.  Node j brings its V row to the rows below it, in the group that owns the slot of j's
    // position, so a row still makes one fma per slot, with the row of its own path.  The nodes go in index order (a loop
    // the whole block shares, kVvUB rows in flight): a row's ancestors come in increasing index, which is increasing depth,
    // which is increasing slot -- the order a row's sum has to keep; the rows' sums do not meet.
    for (int j0 = 0; j0 < n; j0 += kVvUB) {
        v4f vv[kVvUB];
        int tls[kVvUB];
#pragma unroll
        for (int u = 0; u < kVvUB; u++) {
            const int j = min(j0 + u, n - 1);  // clamped: dropped below
            const int tl = a.pos0 + tt->depth[j] - seg0;
            tls[u] = j0 + u < n && tl >= nctx && tl < nk && tl % G == g ? tl : -1;  // -1: not this group's, or not here
            vv[u] = tls[u] >= 0 && c < E ? *(const v4f *)(vbase + (size_t)(a.pos0 + j) * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVvUB; u++)
            if (tls[u] >= 0) {
                const unsigned below = tt->below[min(j0 + u, n - 1)] & act;
#pragma unroll
                for (int i = 0; i < kBatchMax; i++)
                    if ((below >> i) & 1u) {
                        const float wt = sc[i * kVerifySeg + tls[u]];
                        if (wt > 0.0f) {
                            const v4f w4 = {wt, wt, wt, wt};
                            acc[i] = fma4(w4, vv[u], acc[i]);
                        }
                    }
            }
    }
    __syncthreads();
    segment_group_fold<kBatchMax>(s, seg, hs, acc, TPR, sc);
}

// Block (h, i): row i's segments 0 .. (pos0 + depth_i) / kVerifySeg folded in segment order, then the divide
__global__ __launch_bounds__(64) void verify_tree_combine_kernel(const VerifyTreeAttnArgs a)
{
    const int i = blockIdx.y;
    verify_combine_store(a, blockIdx.x, i, (a.pos0 + a.tree->depth[i]) / kVerifySeg + 1);
}

// out[0 .. n) = the rows' next ids.  Every block walks the tree itself (cur = 0; while cur has a child whose token is
// out[cur], go there: at most 15 steps of at most 15 compares) and copies the last node's logits row to dst; block 0
// writes out[n] = a and out[n + 1 + d] = the node walked at depth d, d = 0 .. a.
__global__ __launch_bounds__(256) void verify_tree_accept_kernel(const BatchTable *tab, const VerifyTreeTable *tt, const float *logits,
                                                                 int vocab, int *out, float *dst, int n)
{
    __shared__ int s_a, s_path[kBatchMax];
    if (threadIdx.x == 0) {
        int cur = 0, acc = 0;
        s_path[0] = 0;
        for (;;) {
            int child = -1;
            for (int cnd = cur + 1; cnd < n && child < 0; cnd++)
                if (tt->parent[cnd] == cur && tab->tokens[cnd] == out[cur]) child = cnd;
            if (child < 0) break;
            cur = child;
            s_path[++acc] = cur;
        }
        s_a = acc;
    }
    __syncthreads();
    const int acc = s_a, last = s_path[acc];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < vocab) dst[j] = logits[(size_t)last * vocab + j];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) out[n] = acc;
        if ((int)threadIdx.x <= acc) out[n + 1 + threadIdx.x] = s_path[threadIdx.x];
    }
}

// The accepted path's K / V rows into place: for d = 1 .. a with path[d] != d, physical row pos0 + path[d] -> row
// pos0 + d, in every layer and kv head (res[n] = a, res[n + 1 + d] = path[d]: verify_tree_accept_kernel's).  A thread owns
// one float4 column of one (cache, layer, kv head) across all rows and walks d upwards: path[] increases strictly with
// path[d] >= d, so depth d reads a row above every row written so far.
__global__ __launch_bounds__(256) void verify_tree_compact_kernel(float *kc, float *vc, const int *res, int n, int pos0, int head_size,
                                                                  size_t kv_head_stride, int n_heads_all)
{
    const int E = head_size >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n_heads_all * E) return;
    const int col = (int)(idx % E);
    float *base = (blockIdx.y == 0 ? kc : vc) + (idx / E) * kv_head_stride + 4 * col;  // (layer, kv head) planes are contiguous
    const int acc = res[n];
    for (int d = 1; d <= acc; d++) {
        const int src = res[n + 1 + d];
        if (src != d) *(v4f *)(base + (size_t)(pos0 + d) * head_size) = *(const v4f *)(base + (size_t)(pos0 + src) * head_size);
    }
}

bool verify_tree_args_ok(const VerifyTreeAttnArgs &a, int n, int max_depth)
{
    return n >= 1 && n <= kBatchMax && max_depth >= 0 && max_depth < n && a.pos0 >= 0 && a.tree != nullptr &&
           verify_geom_ok(a, (a.pos0 + max_depth) / kVerifySeg + 1);
}

}  // namespace

hipError_t launch_verify_tree_attention(const VerifyTreeAttnArgs &a, int n, int max_depth, hipStream_t st)
{
    if (!verify_tree_args_ok(a, n, max_depth)) return hipErrorInvalidValue;
    const int nseg = (a.pos0 + max_depth) / kVerifySeg + 1;
    hipLaunchKernelGGL(verify_tree_attention_kernel, dim3(a.n_heads, nseg), dim3(kVaBlock), 0, st, a, n, max_depth);
    return hipGetLastError();
}

hipError_t launch_verify_tree_combine(const VerifyTreeAttnArgs &a, int n, int max_depth, hipStream_t st)
{
    if (!verify_tree_args_ok(a, n, max_depth)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_tree_combine_kernel, dim3(a.n_heads, n), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_verify_tree_accept(const BatchTable *tab, const VerifyTreeTable *tree, const float *logits, int vocab, int *out,
                                     float *dst, int n, hipStream_t st)
{
    if (n < 1 || n > kBatchMax || vocab < 1 || tab == nullptr || tree == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_tree_accept_kernel, dim3((vocab + 255) / 256), dim3(256), 0, st, tab, tree, logits, vocab, out, dst, n);
    return hipGetLastError();
}

hipError_t launch_verify_tree_compact(float *kc, float *vc, const int *res, int n, int pos0, int head_size, size_t kv_head_stride,
                                      int n_layers, int n_kv_heads, hipStream_t st)
{
    if (n < 1 || n > kBatchMax || pos0 < 0 || head_size < 4 || (head_size & 3) != 0 || n_layers < 1 || n_kv_heads < 1)
        return hipErrorInvalidValue;
    if (n < 3) return hipSuccess;  // a path through fewer than three nodes is in place: path[d] == d
    const size_t threads = (size_t)n_layers * n_kv_heads * (head_size >> 2);
    hipLaunchKernelGGL(verify_tree_compact_kernel, dim3((unsigned)((threads + 255) / 256), 2), dim3(256), 0, st, kc, vc, res, n, pos0,
                       head_size, kv_head_stride, n_layers * n_kv_heads);
    return hipGetLastError();
}

}  // namespace l2z
