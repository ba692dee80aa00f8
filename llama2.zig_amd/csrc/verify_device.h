// verify_device.h -- the device bodies of the segment attention: one block serves M QUERY SLOTS from one stream of K / V
// rows, over one segment of kVerifySeg absolute positions, and leaves the flash partials per (slot, segment); a combine
// folds a slot's segments.  What a slot is belongs to the caller: a row of one head for the verify family (l2z_verify in
// verify.hip, l2z_verify_batch in verify_batch.hip, l2z_verify_tree in verify_tree.hip: M = 16), a query head of one row
// for the wide step (wide_decode.hip: M = 1, 2 or 4).  ONE text for all, so that a slot's bits are the same through
// every call: each order below (the lanes' partial dots, a wave's max and sum over the segment, a group's V rows in
// increasing t, the groups in g order, the segments in segment order) depends on head_size, the segment and the slot's
// last visible key alone.
#pragma once
#include "batch_decode.h"
#include "kernel_common.h"

namespace l2z {
namespace {

constexpr int kVaBlock = 256;
constexpr int kVaUB = 4;  // K / V rows a lane has in flight
constexpr int kVaPerLane = kVerifySeg / 64;  // scores of one slot a lane holds in the softmax sweep
static_assert(kVerifySeg % 64 == 0, "a wave sweeps a slot's scores in whole 64-lane steps");
// LDS of a block that serves M slots, in floats: the scores [slot][key], then the groups' V sums, min(M, 4) slots a round
template <int M> constexpr int seg_fold_slots = M < 4 ? M : 4;
template <int M>
constexpr int seg_lds_floats = M * kVerifySeg > seg_fold_slots<M> * 4 * kVaBlock ? M * kVerifySeg : seg_fold_slots<M> * 4 * kVaBlock;

// What every launcher of the verify family asks of the geometry; nseg = the segments the launch covers
inline bool verify_geom_ok(const VerifyAttnGeom &a, int nseg)
{
    return a.head_size >= 4 && a.head_size <= 256 && (a.head_size & 3) == 0 && nseg >= 1 && nseg <= a.seg_cap;
}

// The slots of a block, by strides.  Partials are indexed in units of (row . n_heads + head): index x owns
// part_o[(x * seg_cap + seg) * head_size ..] and part_ml[(x * seg_cap + seg) * 2 ..].
struct SegSlots {
    const float *q;    // slot m's q slice: q + m * q_step
    size_t q_step;
    int see0, see_step;  // slot m sees the keys t <= see0 + m * see_step
    size_t idx0, part_step;  // slot m's partials: index idx0 + m * part_step
    unsigned act;      // bit m: slot m is in use
    float *part_o, *part_ml;
    int seg_cap;
};

// The softmax sweep of segment seg's score rows sc[slot][key], keys 0 .. nk - 1: per slot of s.act, m = max,
// e = exp(s - m) in place, l = sum e (a masked key is -inf, so exactly 0, adding nothing), (m, l) -> s.part_ml.  A wave owns
// slots w, w + 4, ...  Between two barriers of the caller.
template <int M> __device__ __forceinline__ void segment_softmax_sweep(const SegSlots &s, const int seg, const int nk, float *sc)
{
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < M; i += kVaBlock / 64)
        if ((s.act >> i) & 1u) {
            float *r = sc + i * kVerifySeg;
            float sv[kVaPerLane], m = -INFINITY;
#pragma unroll
            for (int j = 0; j < kVaPerLane; j++) {
                sv[j] = lane + 64 * j < nk ? r[lane + 64 * j] : -INFINITY;
                m = fmaxf(m, sv[j]);
            }
            m = wave_max(m);  // finite: the slot sees key 0 of a segment that starts at or below its last visible key
            float l = 0.0f;
#pragma unroll
            for (int j = 0; j < kVaPerLane; j++) {  // a lane's keys in increasing t, then the lanes (wave_sum's fixed order)
                const float e = expf(sv[j] - m);
                if (lane + 64 * j < nk) r[lane + 64 * j] = e;
                l += e;
            }
            l = wave_sum(l);
            if (lane == 0) {
                float *ml = s.part_ml + ((s.idx0 + i * s.part_step) * s.seg_cap + seg) * 2;
                ml[0] = m;
                ml[1] = l;
            }
        }
}

// The lane groups' V sums acc[slot] (group g = threadIdx.x / TPR) combined in g order, min(M, 4) slots per round through
// the score buffer, -> s.part_o for the slots of s.act.  After a barrier of the caller's: the scores are dead.
template <int M>
__device__ __forceinline__ void segment_group_fold(const SegSlots &s, const int seg, const int hs, const v4f (&acc)[M], const int TPR,
                                                   float *sc)
{
    constexpr int FH = seg_fold_slots<M>;
    static_assert(M % FH == 0, "whole rounds");
    const int tid = threadIdx.x, E = hs >> 2, G = kVaBlock / TPR;
    v4f *buf = (v4f *)sc;
#pragma unroll
    for (int r = 0; r < M / FH; r++)
        if ((s.act >> (FH * r)) & ((1u << FH) - 1u)) {
#pragma unroll
            for (int j = 0; j < FH; j++) buf[j * kVaBlock + tid] = acc[FH * r + j];
            __syncthreads();
            if (tid < FH * TPR) {
                const int j = tid / TPR, cc = tid % TPR, i = FH * r + j;
                if (cc < E && ((s.act >> i) & 1u)) {
                    v4f o = buf[j * kVaBlock + cc];
                    for (int gg = 1; gg < G; gg++) o += buf[j * kVaBlock + gg * TPR + cc];
                    *(v4f *)(s.part_o + ((s.idx0 + i * s.part_step) * s.seg_cap + seg) * hs + 4 * cc) = o;
                }
            }
            __syncthreads();
        }
}

// The slots of s over the keys seg * kVerifySeg .. last of ONE stream of K / V rows (kbase / vbase: [t][hs]), last = the
// last key of the segment any slot sees, by a block of kVaBlock threads; sc: seg_lds_floats<M> of LDS.  A K row is read by
// TPR lanes (float4 each) as in batch_attention_kernel, ONCE, and dotted with every slot's q slice (registers); the scores
// of the segment sit in LDS ([slot][key]); a wave owns slots w, w + 4, ... for max / exp / sum; then each V row is read
// once and added into every slot's accumulator.  Keys behind `last` are neither read nor summed.
template <int M>
__device__ __forceinline__ void segment_attention_body(const SegSlots &s, const float *kbase, const float *vbase, const int hs,
                                                       const int seg, const int last, float *sc)
{
    const int tid = threadIdx.x, E = hs >> 2;
    int TPR = 1;
    while (TPR < E) TPR <<= 1;
    const int G = kVaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int seg0 = seg * kVerifySeg;
    const int nk = last - seg0 + 1;  // keys seg0 .. seg0 + nk - 1 are all the block handles
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const float div = sqrtf((float)hs);
    v4f qv[M];
#pragma unroll
    for (int i = 0; i < M; i++) qv[i] = ((s.act >> i) & 1u) && c < E ? *(const v4f *)(s.q + i * s.q_step + 4 * c) : zero;
    // scores sc[i][t - seg0] = q_i . k_t / sqrt(head_size), -inf where slot i does not see t
    for (int tl0 = g; tl0 < nk; tl0 += G * kVaUB) {
        v4f kv[kVaUB];
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int t = min(seg0 + tl0 + G * u, last);  // clamped: dropped below
            kv[u] = c < E ? *(const v4f *)(kbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int tl = tl0 + G * u, t = seg0 + tl;
#pragma unroll
            for (int i = 0; i < M; i++)
                if ((s.act >> i) & 1u) {
                    const float p = lanes_sum(hsum4(fma4(qv[i], kv[u], zero)), TPR);
                    if (c == 0 && tl < nk) sc[i * kVerifySeg + tl] = t <= s.see0 + i * s.see_step ? p / div : -INFINITY;
                }
        }
    }
    __syncthreads();
    segment_softmax_sweep<M>(s, seg, nk, sc);
    __syncthreads();
    // acc_i = sum_t e[i][t] v_t: group g takes t = seg0 + g, + G, ... in increasing t
    v4f acc[M];
#pragma unroll
    for (int i = 0; i < M; i++) acc[i] = zero;
    for (int tl0 = g; tl0 < nk; tl0 += G * kVaUB) {
        v4f vv[kVaUB];
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int t = min(seg0 + tl0 + G * u, last);
            vv[u] = c < E ? *(const v4f *)(vbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int tl = tl0 + G * u;
            if (tl < nk) {
#pragma unroll
                for (int i = 0; i < M; i++)
                    if ((s.act >> i) & 1u) {
                        const float wt = sc[i * kVerifySeg + tl];
                        // an unseen key's weight is exactly 0: skipped, so the sum is that of the seen keys alone.  Where
                        // every slot sees every key of the block (see_step 0, a constant of the caller's) nothing is tested:
                        // a weight of 0 is an underflowed exp there, and its fma leaves the sum's value as it is
                        if (s.see_step == 0 || wt > 0.0f) {
                            const v4f w4 = {wt, wt, wt, wt};
                            acc[i] = fma4(w4, vv[u], acc[i]);
                        }
                    }
            }
        }
    }
    __syncthreads();
    segment_group_fold<M>(s, seg, hs, acc, TPR, sc);
}

// The verify family's slots: up to kBatchMax rows of head h, row i's q at a.q + i * a.ldq, its partials at (i, h).  The
// chain and the batch add what a row sees (see0, see_step) and the rows in use; the tree needs the partials and act alone.
inline __device__ SegSlots verify_slots(const VerifyAttnGeom &a, const int h, const unsigned act)
{
    SegSlots s = {};
    s.q = a.q + (size_t)h * a.head_size; s.q_step = (size_t)a.ldq;
    s.idx0 = (size_t)h; s.part_step = (size_t)a.n_heads;
    s.act = act;
    s.part_o = a.part_o; s.part_ml = a.part_ml; s.seg_cap = a.seg_cap;
    return s;
}

// Head h over the keys t of segment seg that the rows a.pos0 .. a.pos0 + n - 1 of ONE sequence see (t <= pos0 + n - 1);
// sc: seg_lds_floats<kBatchMax>.  a.q, a.part_o and a.part_ml point at the sequence's row 0.
__device__ __forceinline__ void verify_attention_body(const VerifyAttnArgs &a, const int n, const int h, const int seg, float *sc)
{
    const int seg0 = seg * kVerifySeg;
    const int last = min(seg0 + kVerifySeg, a.pos0 + n) - 1;  // the last key of this segment any row of the call sees
    const int i0 = max(0, seg0 - a.pos0);                     // rows below i0 end before this segment
    // rows i0 .. n - 1 (i0 < n: seg0 <= pos0 + n - 1)
    SegSlots s = verify_slots(a, h, (0xFFFFu >> (kBatchMax - n)) & (0xFFFFu << i0));
    s.see0 = a.pos0; s.see_step = 1;
    const size_t head_off = (size_t)(h / a.kv_mul) * a.kv_head_stride;
    segment_attention_body<kBatchMax>(s, a.kc + head_off, a.vc + head_off, a.head_size, seg, last, sc);
}

// One (row, head) of part_o / part_ml, its partials starting at index `base` (in segments), by a lane that owns features
// 4 c .. 4 c + 3: the ns segments folded in segment order (online rescale, UB segments' partials in flight), then the
// divide.  One segment goes through the same arithmetic as many (the fold starts from max = -inf, sum = 0).
template <int UB>
__device__ __forceinline__ v4f segment_combine_body(const float *part_o, const float *part_ml, const size_t base, const int ns,
                                                    const int head_size, const int c)
{
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    float M = -INFINITY, L = 0.0f;
    v4f O = zero;
    for (int s0 = 0; s0 < ns; s0 += UB) {
        v2f ml[UB];
        v4f o[UB];
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const size_t s = base + min(s0 + u, ns - 1);  // clamped: dropped below
            ml[u] = *(const v2f *)(part_ml + s * 2);
            o[u] = *(const v4f *)(part_o + s * head_size + 4 * c);
        }
#pragma unroll
        for (int u = 0; u < UB; u++)
            if (s0 + u < ns) {
                const float mn = fmaxf(M, ml[u].x);
                const float ea = expf(M - mn), eb = expf(ml[u].x - mn);
                L = L * ea + ml[u].y * eb;
                O = O * ea + o[u] * eb;
                M = mn;
            }
    }
    const v4f r = {O.x / L, O.y / L, O.z / L, O.w / L};  // main.zig:704
    return r;
}

// The verify family's combine, block (h, i) of 64 lanes: row i's ns segments -> a.out's row i, head h
constexpr int kVcUB = 8;  // segments' partials a lane has in flight
__device__ __forceinline__ void verify_combine_store(const VerifyAttnGeom &a, const int h, const int i, const int ns)
{
    const int c = threadIdx.x;
    if (c >= (a.head_size >> 2)) return;
    *(v4f *)(a.out + (size_t)i * a.ldo + (size_t)h * a.head_size + 4 * c) =
        segment_combine_body<kVcUB>(a.part_o, a.part_ml, ((size_t)i * a.n_heads + h) * a.seg_cap, ns, a.head_size, c);
}

}  // namespace
}  // namespace l2z
