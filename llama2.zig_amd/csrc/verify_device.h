// verify_device.h -- the device bodies of the position-split verify attention, shared by the kernels of l2z_verify
// (verify.hip: one sequence per launch), l2z_verify_batch (verify_batch.hip: one launch for several sequences) and
// l2z_verify_tree (verify_tree.hip: every row on its own path).  ONE text for all, so that a row's bits are the same
// through every call: each order below (the lanes' partial dots, a wave's max and sum over the segment, a group's V rows in
// increasing t, the groups in g order, the segments in segment order) depends on head_size, the segment and the row's
// position alone.  The rows a block works for are a 16-bit mask `act`, bit i = row i.
#pragma once
#include "batch_decode.h"
#include "kernel_common.h"

namespace l2z {
namespace {

constexpr int kVaBlock = 256;
constexpr int kVaUB = 4;  // K / V rows a lane has in flight
constexpr int kVcUB = 8;  // combine: segments' partials a thread has in flight
constexpr int kVaPerLane = kVerifySeg / 64;  // scores of one row a lane holds in the softmax sweep
constexpr int kVaLds = kBatchMax * kVerifySeg > 16 * kVaBlock ? kBatchMax * kVerifySeg : 16 * kVaBlock;  // floats
static_assert(kVerifySeg % 64 == 0, "a wave sweeps a row of scores in whole 64-lane steps");

// What every launcher of the family asks of the geometry; nseg = the segments the launch covers
inline bool verify_geom_ok(const VerifyAttnGeom &a, int nseg)
{
    return a.head_size >= 4 && a.head_size <= 256 && (a.head_size & 3) == 0 && nseg >= 1 && nseg <= a.seg_cap;
}

// The softmax sweep of segment seg's score rows sc[row][slot], slots 0 .. nk - 1, for head h: per row of act, m = max,
// e = exp(s - m) in place, l = sum e (a masked slot is -inf, so exactly 0, adding nothing), (m, l) -> a.part_ml.  A wave owns
// rows w, w + 4, ...  Between two barriers of the caller.
__device__ __forceinline__ void verify_softmax_sweep(const VerifyAttnGeom &a, const int h, const int seg, const unsigned act,
                                                     const int nk, float *sc)
{
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < kBatchMax; i += kVaBlock / 64)
        if ((act >> i) & 1u) {
            float *r = sc + i * kVerifySeg;
            float sv[kVaPerLane], m = -INFINITY;
#pragma unroll
            for (int j = 0; j < kVaPerLane; j++) {
                sv[j] = lane + 64 * j < nk ? r[lane + 64 * j] : -INFINITY;
                m = fmaxf(m, sv[j]);
            }
            m = wave_max(m);  // finite: the row sees slot 0 of a segment that starts at or below its position
            float l = 0.0f;
#pragma unroll
            for (int j = 0; j < kVaPerLane; j++) {  // a lane's slots in increasing t, then the lanes (wave_sum's fixed order)
                const float e = expf(sv[j] - m);
                if (lane + 64 * j < nk) r[lane + 64 * j] = e;
                l += e;
            }
            l = wave_sum(l);
            if (lane == 0) {
                float *ml = a.part_ml + (((size_t)i * a.n_heads + h) * a.seg_cap + seg) * 2;
                ml[0] = m;
                ml[1] = l;
            }
        }
}

// The lane groups' V sums acc[row] (group g = threadIdx.x / TPR) combined in g order, four rows per round through the
// score buffer, -> a.part_o for the rows of act.  After a barrier of the caller's: the scores are dead.
__device__ __forceinline__ void verify_group_fold(const VerifyAttnGeom &a, const int h, const int seg, const unsigned act,
                                                  const v4f (&acc)[kBatchMax], const int TPR, float *sc)
{
    const int tid = threadIdx.x, hs = a.head_size, E = hs >> 2, G = kVaBlock / TPR;
    v4f *buf = (v4f *)sc;
#pragma unroll
    for (int r = 0; r < kBatchMax / 4; r++)
        if ((act >> (4 * r)) & 0xFu) {
#pragma unroll
            for (int j = 0; j < 4; j++) buf[j * kVaBlock + tid] = acc[4 * r + j];
            __syncthreads();
            if (tid < 4 * TPR) {
                const int j = tid / TPR, cc = tid % TPR, i = 4 * r + j;
                if (cc < E && ((act >> i) & 1u)) {
                    v4f o = buf[j * kVaBlock + cc];
                    for (int gg = 1; gg < G; gg++) o += buf[j * kVaBlock + gg * TPR + cc];
                    *(v4f *)(a.part_o + (((size_t)i * a.n_heads + h) * a.seg_cap + seg) * hs + 4 * cc) = o;
                }
            }
            __syncthreads();
        }
}

// Head h over the keys t of segment seg that the rows a.pos0 .. a.pos0 + n - 1 of ONE sequence see (t <= pos0 + n - 1),
// by a block of kVaBlock threads; sc: kVaLds floats of LDS.  a.q, a.part_o and a.part_ml point at the sequence's row 0.
// A K row is read by TPR lanes (float4 each) as in batch_attention_kernel, ONCE, and dotted with every row's q slice
// (registers); the scores of the segment sit in LDS ([row][key]); a wave owns rows w, w + 4, ... for max / exp / sum; then
// each V row is read once and added into every row's accumulator.
__device__ __forceinline__ void verify_attention_body(const VerifyAttnArgs &a, const int n, const int h, const int seg, float *sc)
{
    const int tid = threadIdx.x;
    const int hs = a.head_size, E = hs >> 2;
    int TPR = 1;
    while (TPR < E) TPR <<= 1;
    const int G = kVaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int seg0 = seg * kVerifySeg;
    const int last = min(seg0 + kVerifySeg, a.pos0 + n) - 1;  // the last key of this segment any row of the call sees
    const int nk = last - seg0 + 1;                           // ... so keys seg0 .. seg0 + nk - 1 are all it handles
    const int i0 = max(0, seg0 - a.pos0);                     // rows below i0 end before this segment
    const unsigned act = (0xFFFFu >> (kBatchMax - n)) & (0xFFFFu << i0);  // rows i0 .. n - 1 (i0 < n: seg0 <= pos0 + n - 1)
    const size_t head_off = (size_t)(h / a.kv_mul) * a.kv_head_stride;
    const float *kbase = a.kc + head_off, *vbase = a.vc + head_off;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const float div = sqrtf((float)hs);
    v4f qv[kBatchMax];
#pragma unroll
    for (int i = 0; i < kBatchMax; i++)
        qv[i] = ((act >> i) & 1u) && c < E ? *(const v4f *)(a.q + (size_t)i * a.ldq + (size_t)h * hs + 4 * c) : zero;
    // scores sc[i][t - seg0] = q_i . k_t / sqrt(head_size), -inf where row i does not see t
    for (int tl0 = g; tl0 < nk; tl0 += G * kVaUB) {
        v4f kv[kVaUB];
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int t = min(seg0 + tl0 + G * u, last);  // clamped: masked below
            kv[u] = c < E ? *(const v4f *)(kbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kVaUB; u++) {
            const int tl = tl0 + G * u, t = seg0 + tl;
#pragma unroll
            for (int i = 0; i < kBatchMax; i++)
                if ((act >> i) & 1u) {
                    const float p = lanes_sum(hsum4(fma4(qv[i], kv[u], zero)), TPR);
                    if (c == 0 && tl < nk) sc[i * kVerifySeg + tl] = t <= a.pos0 + i ? p / div : -INFINITY;
                }
        }
    }
    __syncthreads();
    verify_softmax_sweep(a, h, seg, act, nk, sc);  // (the keys behind the call's last: -inf like the masked ones)
    __syncthreads();
    // acc_i = sum_t e[i][t] v_t: group g takes t = seg0 + g, + G, ... in increasing t
    v4f acc[kBatchMax];
#pragma unroll
    for (int i = 0; i < kBatchMax; i++) acc[i] = zero;
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
                for (int i = 0; i < kBatchMax; i++)
                    if ((act >> i) & 1u) {
                        const float wt = sc[i * kVerifySeg + tl];
                        if (wt > 0.0f) {  // an unseen key's weight is 0: skipped, so the sum is that of the seen keys alone
                            const v4f w4 = {wt, wt, wt, wt};
                            acc[i] = fma4(w4, vv[u], acc[i]);
                        }
                    }
            }
        }
    }
    __syncthreads();
    verify_group_fold(a, h, seg, act, acc, TPR, sc);
}

// Head h of the row whose partials start at index `base` of part_ml / part_o (in segments), by 64 threads: its ns
// segments folded in segment order (online rescale), then the divide, into o[0 .. head_size).  One segment goes through
// the same arithmetic as many (the fold starts from max = -inf, sum = 0).
__device__ __forceinline__ void verify_combine_body(const float *part_o, const float *part_ml, const size_t base, const int ns,
                                                    const int head_size, float *o_row)
{
    for (int d = threadIdx.x; d < head_size; d += 64) {
        float M = -INFINITY, L = 0.0f, O = 0.0f;
        for (int s0 = 0; s0 < ns; s0 += kVcUB) {  // kVcUB segments' partials in flight, folded in segment order
            float m[kVcUB], l[kVcUB], o[kVcUB];
#pragma unroll
            for (int u = 0; u < kVcUB; u++) {
                const size_t s = base + min(s0 + u, ns - 1);  // clamped: dropped below
                m[u] = part_ml[s * 2];
                l[u] = part_ml[s * 2 + 1];
                o[u] = part_o[s * head_size + d];
            }
#pragma unroll
            for (int u = 0; u < kVcUB; u++)
                if (s0 + u < ns) {
                    const float mn = fmaxf(M, m[u]);
                    const float ea = expf(M - mn), eb = expf(m[u] - mn);
                    L = L * ea + l[u] * eb;
                    O = O * ea + o[u] * eb;
                    M = mn;
                }
        }
        o_row[d] = O / L;
    }
}

}  // namespace
}  // namespace l2z
