// kv8_verify_attention.hip -- causal segment attention of up to kBatchMax = 16 rows of ONE sequence over its int8 K / V rows
// (kv8.h, kv8_layout.h): what verify_attention_body (verify_device.h) is to the f32 cache, behind
// l2z_verify_kv8.  Row i stands at position pos0 + i and sees the keys t <= pos0 + i.
//
// Block map   block (kv head, segment of kVerifySeg = 64 absolute positions, [sequence: one today]), 256 threads.  The block
//             requests the segment's K dwords, its V dwords and its 2 x 64 scales ONCE and keeps the dwords in registers; it
//             then walks the kv head's kv_mul query heads one after the other, each with 16 row slots.  So a segment's
//             bytes are read once per kv head for every row AND every query head of the call -- sixteen one-row blocks
//             of kv8_attention read them sixteen times.  Segments above pos0 + n - 1 are not launched.
// Lane map    kv8_attention's: TPR = kv8_lanes(head_size) lanes a key row, a dword (four values) a lane; G = 256 / TPR rows
//             side by side; group g takes the keys seg0 + g, + G, ... in batches of kKv8UB = 8 dwords a lane.  The
//             segment is NB = 1 batch up to head_size 128 and NB = 2 above; all NB are in flight at once and stay.
// Loads       K's batches first; then the 64 K scales and 64 V scales by waves 0 and 1 into LDS; then head 0's q slices;
//             V's batches are requested BEFORE the first softmax sweep and wait behind it.
// Per head    scores  (q_i . k_t) by the chain fmaf(q.w, k3, fmaf(q.z, k2, fmaf(q.y, k1, fmaf(q.x, k0, 0)))), lanes_sum
//                     over TPR, then (dot * ks[t]) / sqrt(head_size) -- or -INFINITY, WRITTEN, where t > pos0 + i: a key
//                     the row may not see never reaches it through arithmetic, so a NaN scale there stays out.
//             softmax segment_softmax_sweep, unchanged (a masked key: e = exp(-inf - m) = 0 exactly, adding nothing).
//             V       acc = fmaf(e * vs[t], f32(v), acc), keys of e == 0 skipped (segment_attention_body's test: the sum is
//                     that of the seen keys alone); group g in increasing t; segment_group_fold, unchanged, in g order.
// So row i's partials of a segment are, operation for operation, those kv8_attention leaves for a one-row sequence at
// position pos0 + i: its block sees nk' = min(nk, pos0 + i - seg0 + 1) keys where this one sees nk and writes -inf
// behind nk' -- which is what the sweep itself puts there.  The partials go to the wide step's layout
// (row . n_heads + head); wide_combine, as it stands, folds them.  Vector loads and stores only; every FMA is an explicit fmaf.
#include "kv8.h"

#include "kernel_common.h"
#include "kv8_device.h"
#include "verify_device.h"

namespace l2z {
namespace {

constexpr int kKv8UB = 8;   // dwords of K (and of V) a lane has in flight per batch (kv8_attention's)

struct Kv8VerifyArgs {
    const float *q;           // the sequence's row 0
    const Kv8Seq *seq;        // device: the sequences' arrays; this launch serves seq[seq_i] alone
    float *part_o, *part_ml;  // [kWideMax, n_heads, seg_cap, head_size] and [..., 2], indexed by the row
    size_t layer_off, kv_head_stride;   // in values; a scale stands at (the value's index) / head_size
    int seq_i, pos0, n;       // rows 0 .. n - 1 at positions pos0 ..
    int ldq, n_heads, kv_mul, head_size, seg_cap;
};

template <int NB>
__global__ __launch_bounds__(kVaBlock) void kv8_verify_attention(const Kv8VerifyArgs a)
{
    constexpr int M = kBatchMax, U = NB * kKv8UB;
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<M>];   // scores [row][key], then the groups' V sums
    __shared__ float s_ks[kVerifySeg], s_vs[kVerifySeg];
    const int kvh = blockIdx.x, seg = blockIdx.y, tid = threadIdx.x;
    const int seg0 = seg * kVerifySeg;
    const int top = a.pos0 + a.n - 1;   // the last key any row of the call sees
    if (seg0 > top) return;             // (uniform, before any barrier)
    const int hs = a.head_size, E = hs >> 2, TPR = kv8_lanes(hs);
    const int G = kVaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int nk = min(seg0 + kVerifySeg - 1, top) - seg0 + 1;   // keys seg0 .. seg0 + nk - 1 are all the block handles
    const int i0 = max(0, seg0 - a.pos0);                        // rows below i0 end before this segment (i0 < n)
    const unsigned act = (0xFFFFu >> (M - a.n)) & (0xFFFFu << i0);
    const Kv8Seq sq = a.seq[a.seq_i];
    const size_t head_off = a.layer_off + (size_t)kvh * a.kv_head_stride + (size_t)seg0 * (size_t)hs;   // the segment's first row
    const int8_t *kbase = sq.k8 + head_off + 4 * c, *vbase = sq.v8 + head_off + 4 * c;
    const bool lane_on = c < E;

    // ---- requests: K's batches, the scales; V's follow behind head 0's scores ----
    int kw[U], vw[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int tl = g + G * u;
        kw[u] = lane_on && tl < nk ? *(const int *)(kbase + (size_t)tl * hs) : 0;
    }
    if (tid < 2 * kVerifySeg) {   // waves 0 and 1: the K scales, the V scales
        const int tl = tid & (kVerifySeg - 1);
        const float *from = (tid < kVerifySeg ? sq.ks : sq.vs) + head_off / (size_t)hs;
        (tid < kVerifySeg ? s_ks : s_vs)[tl] = tl < nk ? from[tl] : 0.0f;
    }
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const float div = sqrtf((float)hs);

    for (int hq = 0; hq < a.kv_mul; hq++) {
        const int h = kvh * a.kv_mul + hq;
        SegSlots s = {};
        s.idx0 = (size_t)h; s.part_step = (size_t)a.n_heads;   // row i's partials: index i * n_heads + h
        s.act = act;
        s.part_o = a.part_o; s.part_ml = a.part_ml; s.seg_cap = a.seg_cap;

        v4f qv[M];
#pragma unroll
        for (int i = 0; i < M; i++)
            qv[i] = ((act >> i) & 1u) && lane_on ? *(const v4f *)(a.q + (size_t)i * a.ldq + (size_t)h * hs + 4 * c) : zero;
        if (hq == 0) __syncthreads();   // the scales stand (later heads: the fold's last barrier is behind them)

        // ---- scores sc[i][t - seg0] = (q_i . k_t) * ks[t] / sqrt(head_size), -inf where row i does not see t ----
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int tl = g + G * u;
            const v4f kf = kv8_unpack(kw[u]);
#pragma unroll
            for (int i = 0; i < M; i++)
                if ((act >> i) & 1u) {
                    float p = fmaf(qv[i].x, kf.x, 0.0f);
                    p = fmaf(qv[i].y, kf.y, p);
                    p = fmaf(qv[i].z, kf.z, p);
                    p = fmaf(qv[i].w, kf.w, p);
                    p = lanes_sum(p, TPR);
                    if (c == 0 && tl < nk) sc[i * kVerifySeg + tl] = seg0 + tl <= a.pos0 + i ? (p * s_ks[tl]) / div : -INFINITY;
                }
        }
        if (hq == 0) {   // V's batches, requested before the sweep
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int tl = g + G * u;
                vw[u] = lane_on && tl < nk ? *(const int *)(vbase + (size_t)tl * hs) : 0;
            }
        }
        __syncthreads();
        segment_softmax_sweep<M>(s, seg, nk, sc);
        __syncthreads();

        // ---- acc_i = sum_t (e[i][t] * vs[t]) f32(v_t): group g takes t = seg0 + g, + G, ... in increasing t ----
        v4f acc[M];
#pragma unroll
        for (int i = 0; i < M; i++) acc[i] = zero;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int tl = g + G * u;
            if (tl < nk) {
                const v4f vf = kv8_unpack(vw[u]);
                const float vs = s_vs[tl];
#pragma unroll
                for (int i = 0; i < M; i++)
                    if ((act >> i) & 1u) {
                        const float e = sc[i * kVerifySeg + tl];
                        if (e > 0.0f) {   // an unseen key's weight is exactly 0: skipped, its scale never multiplied in
                            const float wt = e * vs;
                            const v4f w4 = {wt, wt, wt, wt};
                            acc[i] = fma4(w4, vf, acc[i]);
                        }
                    }
            }
        }
        __syncthreads();
        segment_group_fold<M>(s, seg, hs, acc, TPR, sc);   // (ends behind a barrier: the next head may write its scores)
    }
}

}  // namespace

hipError_t launch_kv8_verify_attention(const RaggedLayer &L, const WideAttn &wa, const Kv8Seq *seq8, int seq, int pos0,
                                       bool *planes_written)
{
    if (planes_written) *planes_written = false;
    const int n = L.P, kv_mul = L.kv_mul, hs = L.head_size;
    if (n < 1 || n > kBatchMax || pos0 < 0 || seq < 0 || hs < 4 || hs > 256 || (hs & 3) || L.n_heads < 1 || kv_mul < 1 ||
        L.n_heads % kv_mul != 0 || (L.ldq & 3) || (((uintptr_t)L.q | (uintptr_t)wa.part) & 15) || (L.layer_off & 3) ||
        (L.kv_head_stride & 3) || wa.tab == nullptr || wa.part == nullptr || seq8 == nullptr ||
        wa.n_seg != (pos0 + n - 1) / kVerifySeg + 1 || wa.n_seg > wa.seg_cap || wa.page_floats != 0)
        return hipErrorInvalidValue;
    Kv8VerifyArgs a = {};
    a.q = L.q; a.seq = seq8; a.seq_i = seq; a.pos0 = pos0; a.n = n;
    a.part_o = wa.part;
    a.part_ml = wa.part + (size_t)kWideMax * L.n_heads * wa.seg_cap * hs;
    a.layer_off = L.layer_off; a.kv_head_stride = L.kv_head_stride;
    a.ldq = L.ldq; a.n_heads = L.n_heads; a.kv_mul = kv_mul; a.head_size = hs; a.seg_cap = wa.seg_cap;
    const dim3 grid(L.n_heads / kv_mul, wa.n_seg);
    if (hs <= 128) hipLaunchKernelGGL(kv8_verify_attention<1>, grid, dim3(kVaBlock), 0, L.st, a);
    else hipLaunchKernelGGL(kv8_verify_attention<2>, grid, dim3(kVaBlock), 0, L.st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_combine(L.out, L.ldo, wa, n, L.n_heads, hs, L.st, L.x3, L.kp, planes_written);
}

}  // namespace l2z
