// kv8_attention.hip -- the read side of the int8 KV cache (kv8.h, kv8_layout.h): decode attention of up to
// kWideMax one-row sequences, each over its own int8 K / V rows and their scales.
//
// The frame is wide_attention's (wide_decode.hip): block (kv head x part of up to 4 query heads, segment of kVerifySeg = 64
// absolute positions, row), 256 threads; a block past its row's last segment returns; the flash partials (max, sum e,
// sum e v) per (row, head, segment) go to the wide step's layout and wide_combine, as it stands, folds them.
//
// Inside the block the design is the int8 one.  A segment of one kv head is 64 x head_size BYTES (8 KB at head_size 128),
// so a lane holds a whole key row's share as ONE dword and the whole segment is in flight at once:
//   lane map   TPR = kv8_lanes(head_size) lanes a key row, a dword (four values) a lane; G = 256 / TPR rows side by side;
//              group g takes the keys seg0 + g, + G, ... in batches of kKv8UB = 8 dwords a lane (head_size 128: G = 8, ONE
//              batch is the segment; 256: two batches; below 128 a batch has rows to spare, which are not requested).
//   loads      K's batch is requested first; then the segment's 64 K scales and 64 V scales, one 256-byte read each by waves
//              0 and 1 into LDS; then q.  V's first batch is requested BEFORE the softmax sweep and waits behind it.
//   scores     the four bytes are converted exactly (kv8_unpack), the lane's partial dot is the chain
//              fmaf(q.w, k3, fmaf(q.z, k2, fmaf(q.y, k1, fmaf(q.x, k0, 0)))), the lanes' sum is lanes_sum over TPR (the
//              segment body's order), then (dot * ks[t]) / sqrt(head_size) by lane 0 of the group into sc[slot][key].
//   softmax    segment_softmax_sweep, unchanged: a wave a slot, m, e in place, l, (m, l) -> the partials.
//   weighted V acc = fmaf(e * vs[t], f32(v), acc) per value: the key's weight and scale are multiplied once a (slot, key).
//              Group g adds its keys in increasing t; segment_group_fold, unchanged, adds the groups in g order.
// Every order above is a function of head_size, the segment and the row's own position alone.  A row's result depends on
// its own q, its own cache rows 0 .. pos and its position: no block touches two sequences.  A key beyond the row's
// position is neither read nor summed, nor is its scale.  Vector loads and stores only; every FMA is an explicit fmaf.
#include "kv8.h"

#include "kernel_common.h"
#include "kv8_device.h"
#include "verify_device.h"

namespace l2z {
namespace {

constexpr int kKv8UB = 8;        // dwords of K (and of V) a lane has in flight
constexpr int kKv8HeadsMax = 4;  // query heads of one kv head a block serves (wide_attention's kWaHeadsMax)

struct Kv8AttnArgs {
    const float *q;
    const int32_t *pos;       // [rows] a row's position
    const Kv8Seq *seq;        // [rows] a row's arrays
    float *part_o, *part_ml;  // [kWideMax, n_heads, seg_cap, head_size] and [..., 2]
    size_t layer_off, kv_head_stride;   // in values; a scale stands at (the value's index) / head_size
    int ldq, n_heads, kv_mul, head_size, seg_cap;
};

template <int MQ>
__global__ __launch_bounds__(kVaBlock) void kv8_attention(const Kv8AttnArgs a)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<MQ>];
    __shared__ float s_ks[kVerifySeg], s_vs[kVerifySeg];
    const int row = blockIdx.z, seg = blockIdx.y, tid = threadIdx.x;
    const int pos = a.pos[row];
    const int seg0 = seg * kVerifySeg;
    if (seg0 > pos) return;  // past this row's last segment (uniform, before any barrier)
    const int parts = (a.kv_mul + MQ - 1) / MQ;
    const int kvh = blockIdx.x / parts, hq0 = (blockIdx.x % parts) * MQ;
    const int h0 = kvh * a.kv_mul + hq0;
    const int nq = min(MQ, a.kv_mul - hq0);
    SegSlots s = {};
    s.see0 = pos; s.see_step = 0;
    s.idx0 = (size_t)row * a.n_heads + h0; s.part_step = 1;
    s.act = (1u << nq) - 1u;
    s.part_o = a.part_o; s.part_ml = a.part_ml; s.seg_cap = a.seg_cap;

    const int hs = a.head_size, E = hs >> 2, TPR = kv8_lanes(hs);
    const int G = kVaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int last = min(seg0 + kVerifySeg - 1, pos);
    const int nk = last - seg0 + 1;  // keys seg0 .. seg0 + nk - 1 are all the block handles
    const Kv8Seq sq = a.seq[row];
    const size_t head_off = a.layer_off + (size_t)kvh * a.kv_head_stride + (size_t)seg0 * (size_t)hs;   // the segment's first row
    const int8_t *kbase = sq.k8 + head_off + 4 * c, *vbase = sq.v8 + head_off + 4 * c;
    const bool lane_on = c < E;

    // ---- requests: K's first batch, the scales, q ----
    int kw[kKv8UB];
#pragma unroll
    for (int u = 0; u < kKv8UB; u++) {
        const int tl = g + G * u;
        kw[u] = lane_on && tl < nk ? *(const int *)(kbase + (size_t)tl * hs) : 0;
    }
    if (tid < 2 * kVerifySeg) {   // waves 0 and 1: the K scales, the V scales
        const int tl = tid & (kVerifySeg - 1);
        const float *from = (tid < kVerifySeg ? sq.ks : sq.vs) + head_off / (size_t)hs;
        (tid < kVerifySeg ? s_ks : s_vs)[tl] = tl < nk ? from[tl] : 0.0f;
    }
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    v4f qv[MQ];
#pragma unroll
    for (int i = 0; i < MQ; i++)
        qv[i] = ((s.act >> i) & 1u) && lane_on ? *(const v4f *)(a.q + (size_t)row * a.ldq + (size_t)(h0 + i) * hs + 4 * c) : zero;
    __syncthreads();   // the scales stand

    // ---- scores sc[i][t - seg0] = (q_i . k_t) * ks[t] / sqrt(head_size) ----
    const float div = sqrtf((float)hs);
    for (int tl0 = g; tl0 < nk; tl0 += G * kKv8UB) {
        if (tl0 != g) {   // (head sizes above 128: the second batch)
#pragma unroll
            for (int u = 0; u < kKv8UB; u++) {
                const int tl = tl0 + G * u;
                kw[u] = lane_on && tl < nk ? *(const int *)(kbase + (size_t)tl * hs) : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < kKv8UB; u++) {
            const int tl = tl0 + G * u;
            const v4f kf = kv8_unpack(kw[u]);
#pragma unroll
            for (int i = 0; i < MQ; i++)
                if ((s.act >> i) & 1u) {
                    float p = fmaf(qv[i].x, kf.x, 0.0f);
                    p = fmaf(qv[i].y, kf.y, p);
                    p = fmaf(qv[i].z, kf.z, p);
                    p = fmaf(qv[i].w, kf.w, p);
                    p = lanes_sum(p, TPR);
                    if (c == 0 && tl < nk) sc[i * kVerifySeg + tl] = (p * s_ks[tl]) / div;
                }
        }
    }
    // V's first batch, requested before the sweep
    int vw[kKv8UB];
#pragma unroll
    for (int u = 0; u < kKv8UB; u++) {
        const int tl = g + G * u;
        vw[u] = lane_on && tl < nk ? *(const int *)(vbase + (size_t)tl * hs) : 0;
    }
    __syncthreads();
    segment_softmax_sweep<MQ>(s, seg, nk, sc);
    __syncthreads();

    // ---- acc_i = sum_t (e[i][t] * vs[t]) f32(v_t): group g takes t = seg0 + g, + G, ... in increasing t ----
    v4f acc[MQ];
#pragma unroll
    for (int i = 0; i < MQ; i++) acc[i] = zero;
    for (int tl0 = g; tl0 < nk; tl0 += G * kKv8UB) {
        if (tl0 != g) {
#pragma unroll
            for (int u = 0; u < kKv8UB; u++) {
                const int tl = tl0 + G * u;
                vw[u] = lane_on && tl < nk ? *(const int *)(vbase + (size_t)tl * hs) : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < kKv8UB; u++) {
            const int tl = tl0 + G * u;
            if (tl < nk) {
                const v4f vf = kv8_unpack(vw[u]);
                const float vs = s_vs[tl];
#pragma unroll
                for (int i = 0; i < MQ; i++)
                    if ((s.act >> i) & 1u) {
                        const float wt = sc[i * kVerifySeg + tl] * vs;
                        const v4f w4 = {wt, wt, wt, wt};
                        acc[i] = fma4(w4, vf, acc[i]);
                    }
            }
        }
    }
    __syncthreads();
    segment_group_fold<MQ>(s, seg, hs, acc, TPR, sc);
}

}  // namespace

hipError_t launch_kv8_attention(const RaggedLayer &L, const WideAttn &wa, const Kv8Seq *seq8, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    const int n = L.P, kv_mul = L.kv_mul, hs = L.head_size;
    if (n < 1 || n > kWideMax || hs < 4 || hs > 256 || (hs & 3) || L.n_heads < 1 || kv_mul < 1 || L.n_heads % kv_mul != 0 ||
        (L.ldq & 3) || (((uintptr_t)L.q | (uintptr_t)wa.part) & 15) || (L.layer_off & 3) || (L.kv_head_stride & 3) ||
        wa.tab == nullptr || wa.part == nullptr || seq8 == nullptr || wa.n_seg < 1 || wa.n_seg > wa.seg_cap || wa.page_floats != 0)
        return hipErrorInvalidValue;
    Kv8AttnArgs a = {};
    a.q = L.q; a.pos = wa.tab->pos; a.seq = seq8;
    a.part_o = wa.part;
    a.part_ml = wa.part + (size_t)kWideMax * L.n_heads * wa.seg_cap * hs;
    a.layer_off = L.layer_off; a.kv_head_stride = L.kv_head_stride;
    a.ldq = L.ldq; a.n_heads = L.n_heads; a.kv_mul = kv_mul; a.head_size = hs; a.seg_cap = wa.seg_cap;
    const int mq = kv_mul == 1 ? 1 : kv_mul == 2 ? 2 : kKv8HeadsMax;
    const dim3 grid(L.n_heads / kv_mul * ((kv_mul + mq - 1) / mq), wa.n_seg, n);
    switch (mq) {
        case 1: hipLaunchKernelGGL(kv8_attention<1>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 2: hipLaunchKernelGGL(kv8_attention<2>, grid, dim3(kVaBlock), 0, L.st, a); break;
        default: hipLaunchKernelGGL(kv8_attention<kKv8HeadsMax>, grid, dim3(kVaBlock), 0, L.st, a); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_combine(L.out, L.ldo, wa, n, L.n_heads, hs, L.st, L.x3, L.kp, planes_written);
}

}  // namespace l2z
