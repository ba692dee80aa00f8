// wide_decode.hip -- the kernels l2z_transformer_wide adds to the ragged prompt pass (wide_decode.h; host side:
// wide_host.cpp): decode attention for many one-query sequences, each on its own cache, split over positions in the verify
// family's fixed segments of absolute positions, and the launch that hands the logits matrix back to the runstates.
//
// A row's results depend on that row's q, its own cache rows 0 .. pos and its own position only: no block touches two
// sequences, and every order below (the lanes' partial dots, a wave's max and sum over the segment, a group's V rows in
// increasing t, the groups in g order, the segments in segment order) is a function of head_size, the segment and the
// row's position.  Vector loads and stores only; every FMA is an explicit fmaf.
#include "wide_decode.h"

#include "kernel_common.h"
#include "prefill_common.h"

namespace l2z {
namespace {

constexpr int kWaBlock = 256;
constexpr int kWaUB = 4;        // K / V rows a lane has in flight
constexpr int kWcUB = 4;        // combine: segments' partials a thread has in flight
constexpr int kWaHeadsMax = 4;  // query heads of one kv head a block serves (8: 256 VGPRs, one wave per SIMD)
static_assert(kVerifySeg == 64, "a wave sweeps a head's scores of one segment in one 64-lane step");

struct WideAttnArgs {
    const float *q;
    float *out;
    const WideTable *tab;
    float *part_o, *part_ml;  // [kWideMax, n_heads, seg_cap, head_size] and [..., 2]
    size_t layer_off, kv_head_stride;
    int ldq, ldo, n_heads, kv_mul, head_size, seg_cap;
    __bf16 *x3;  // != null: out's planes of bf16 terms too
    int kp;
};

// Block (kv head x part, segment, row); MQ = query heads per block (a part = MQ consecutive heads of the kv head: one part
// while kv_mul <= kWaHeadsMax).  A K row is read by TPR lanes (float4 each) ONCE and dotted with every head's q slice
// (registers); the segment's scores sit in LDS ([head][key]); a wave owns heads w, w + 4 for max / exp / sum; then each V
// row is read once and added into every head's accumulator; the lane groups' sums are combined in g order through LDS.
// Keys behind the row's position are not part of the segment (nk): they are neither read nor summed.
template <int MQ>
__global__ __launch_bounds__(kWaBlock) void wide_attention(const WideAttnArgs a)
{
    constexpr int FH = MQ < 4 ? MQ : 4;  // heads per round of the group fold
    __shared__ __attribute__((aligned(16))) float sc[FH * 4 * kWaBlock];
    static_assert(MQ * kVerifySeg <= FH * 4 * kWaBlock && MQ % FH == 0, "scores and fold rounds share the buffer");
    const int row = blockIdx.z, seg = blockIdx.y;
    const int pos = a.tab->pos[row];
    const int seg0 = seg * kVerifySeg;
    if (seg0 > pos) return;  // past this row's last segment (uniform, before any barrier)
    const int parts = (a.kv_mul + MQ - 1) / MQ;
    const int kvh = blockIdx.x / parts, hq0 = (blockIdx.x % parts) * MQ;
    const int h0 = kvh * a.kv_mul + hq0;
    const int nq = min(MQ, a.kv_mul - hq0);
    const int tid = threadIdx.x, hs = a.head_size, E = hs >> 2;
    int TPR = 1;
    while (TPR < E) TPR <<= 1;
    const int G = kWaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int nk = min(kVerifySeg, pos - seg0 + 1);  // keys seg0 .. seg0 + nk - 1
    const int last = seg0 + nk - 1;
    const RaggedSeq sq = a.tab->seq[row];
    const size_t head_off = a.layer_off + (size_t)kvh * a.kv_head_stride;
    const float *kbase = sq.kc + head_off, *vbase = sq.vc + head_off;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const float div = sqrtf((float)hs);
    v4f qv[MQ];
#pragma unroll
    for (int m = 0; m < MQ; m++)
        qv[m] = m < nq && c < E ? *(const v4f *)(a.q + (size_t)row * a.ldq + (size_t)(h0 + m) * hs + 4 * c) : zero;
    // scores sc[m][t - seg0] = q_m . k_t / sqrt(head_size)
    for (int tl0 = g; tl0 < nk; tl0 += G * kWaUB) {
        v4f kv[kWaUB];
#pragma unroll
        for (int u = 0; u < kWaUB; u++) {
            const int t = min(seg0 + tl0 + G * u, last);  // clamped: dropped below
            kv[u] = c < E ? *(const v4f *)(kbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kWaUB; u++) {
            const int tl = tl0 + G * u;
#pragma unroll
            for (int m = 0; m < MQ; m++)
                if (m < nq) {
                    const float p = lanes_sum(hsum4(fma4(qv[m], kv[u], zero)), TPR);
                    if (c == 0 && tl < nk) sc[m * kVerifySeg + tl] = p / div;
                }
        }
    }
    __syncthreads();
    {   // per head: m = max, e = exp(s - m) in place, l = sum e (wave_sum's fixed order) -> part_ml
        const int lane = tid & 63;
        for (int m = tid >> 6; m < nq; m += kWaBlock / 64) {
            float *r = sc + m * kVerifySeg;
            const float s = lane < nk ? r[lane] : -INFINITY;
            const float mx = wave_max(s);  // finite: key seg0 is at or below the row's position
            const float e = expf(s - mx);  // a lane without a key: exactly 0
            if (lane < nk) r[lane] = e;
            const float l = wave_sum(e);
            if (lane == 0) {
                const v2f ml = {mx, l};
                *(v2f *)(a.part_ml + (((size_t)row * a.n_heads + h0 + m) * a.seg_cap + seg) * 2) = ml;
            }
        }
    }
    __syncthreads();
    // acc_m = sum_t e[m][t] v_t: group g takes t = seg0 + g, + G, ... in increasing t
    v4f acc[MQ];
#pragma unroll
    for (int m = 0; m < MQ; m++) acc[m] = zero;
    for (int tl0 = g; tl0 < nk; tl0 += G * kWaUB) {
        v4f vv[kWaUB];
#pragma unroll
        for (int u = 0; u < kWaUB; u++) {
            const int t = min(seg0 + tl0 + G * u, last);
            vv[u] = c < E ? *(const v4f *)(vbase + (size_t)t * hs + 4 * c) : zero;
        }
#pragma unroll
        for (int u = 0; u < kWaUB; u++) {
            const int tl = tl0 + G * u;
            if (tl < nk) {
#pragma unroll
                for (int m = 0; m < MQ; m++)
                    if (m < nq) {
                        const float wt = sc[m * kVerifySeg + tl];
                        const v4f w4 = {wt, wt, wt, wt};
                        acc[m] = fma4(w4, vv[u], acc[m]);
                    }
            }
        }
    }
    __syncthreads();  // the scores are dead: the buffer takes the groups' sums, FH heads per round
    v4f *buf = (v4f *)sc;
#pragma unroll
    for (int r = 0; r < MQ; r += FH)
        if (r < nq) {
#pragma unroll
            for (int j = 0; j < FH; j++) buf[j * kWaBlock + tid] = acc[r + j];
            __syncthreads();
            if (tid < FH * TPR) {
                const int j = tid / TPR, cc = tid % TPR, m = r + j;
                if (cc < E && m < nq) {
                    v4f o = buf[j * kWaBlock + cc];
                    for (int gg = 1; gg < G; gg++) o += buf[j * kWaBlock + gg * TPR + cc];
                    *(v4f *)(a.part_o + (((size_t)row * a.n_heads + h0 + m) * a.seg_cap + seg) * hs + 4 * cc) = o;
                }
            }
            __syncthreads();
        }
}

// Block (head, row), lane c = four features: the row's segments 0 .. pos / kVerifySeg folded in segment order (online
// rescale from max = -inf, sum = 0, so one segment goes through the same arithmetic as many), then the divide.
__global__ __launch_bounds__(64) void wide_combine(const WideAttnArgs a)
{
    const int h = blockIdx.x, row = blockIdx.y, c = threadIdx.x, hs = a.head_size;
    if (c >= (hs >> 2)) return;
    const int ns = a.tab->pos[row] / kVerifySeg + 1;
    const size_t base = ((size_t)row * a.n_heads + h) * a.seg_cap;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    float M = -INFINITY, L = 0.0f;
    v4f O = zero;
    for (int s0 = 0; s0 < ns; s0 += kWcUB) {
        v2f ml[kWcUB];
        v4f o[kWcUB];
#pragma unroll
        for (int u = 0; u < kWcUB; u++) {
            const size_t s = base + min(s0 + u, ns - 1);  // clamped: dropped below
            ml[u] = *(const v2f *)(a.part_ml + s * 2);
            o[u] = *(const v4f *)(a.part_o + s * hs + 4 * c);
        }
#pragma unroll
        for (int u = 0; u < kWcUB; u++)
            if (s0 + u < ns) {
                const float mn = fmaxf(M, ml[u].x);
                const float ea = expf(M - mn), eb = expf(ml[u].x - mn);
                L = L * ea + ml[u].y * eb;
                O = O * ea + o[u] * eb;
                M = mn;
            }
    }
    const v4f r = {O.x / L, O.y / L, O.z / L, O.w / L};  // main.zig:704
    *(v4f *)(a.out + (size_t)row * a.ldo + (size_t)h * hs + 4 * c) = r;
    if (a.x3) planes_store4(a.x3, a.kp, row, h * hs + 4 * c, r);
}

// Block = row, 1024 threads: the copy, and the argmax of what was copied.  A thread takes its elements in increasing
// index order (strict '>' keeps the lowest index of equal values); the candidates combine by (value, then lower index).
__global__ __launch_bounds__(1024) void wide_logits_out(const float *logits, int ld, const WideTable *tab, int vocab, int *next)
{
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float *src = logits + (size_t)row * ld;
    float *dst = tab->logits[row];
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int n4 = vec ? vocab >> 2 : 0;
    ArgmaxCand cand;
    for (int i = tid; i < n4; i += 1024) {
        const v4f v = ((const v4f *)src)[i];
        ((v4f *)dst)[i] = v;
        argmax_take(cand, v.x, 4 * i);
        argmax_take(cand, v.y, 4 * i + 1);
        argmax_take(cand, v.z, 4 * i + 2);
        argmax_take(cand, v.w, 4 * i + 3);
    }
    for (int i = 4 * n4 + tid; i < vocab; i += 1024) {
        const float v = src[i];
        dst[i] = v;
        argmax_take(cand, v, i);
    }
    argmax_wave_fold(cand);
    if ((tid & 63) == 0) { s_val[tid >> 6] = cand.v; s_idx[tid >> 6] = cand.i; }
    __syncthreads();
    if (tid == 0 && next != nullptr) {
        argmax_fold_waves(cand, s_val, s_idx, 16);
        next[row] = cand.i == kNoCandidate ? 0 : cand.i;
    }
}

}  // namespace

hipError_t launch_wide_attention(const float *q, int ldq, float *out, int ldo, const WideAttn &wa, int n, int n_heads,
                                 int head_size, size_t layer_off, size_t kv_head_stride, int kv_mul, hipStream_t st, void *x3,
                                 int kp, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    if (n < 1 || n > kWideMax || head_size < 4 || head_size > 256 || (head_size & 3) || kv_mul < 1 || n_heads < 1 ||
        n_heads % kv_mul != 0 || wa.tab == nullptr || wa.part == nullptr || wa.n_seg < 1 || wa.n_seg > wa.seg_cap ||
        (ldq & 3) || (ldo & 3) || (((uintptr_t)q | (uintptr_t)out | (uintptr_t)wa.part) & 15) || (layer_off & 3) ||
        (kv_head_stride & 3))
        return hipErrorInvalidValue;
    WideAttnArgs a = {};
    a.q = q; a.out = out; a.tab = wa.tab;
    a.part_o = wa.part;
    a.part_ml = wa.part + (size_t)kWideMax * n_heads * wa.seg_cap * head_size;
    a.layer_off = layer_off; a.kv_head_stride = kv_head_stride;
    a.ldq = ldq; a.ldo = ldo; a.n_heads = n_heads; a.kv_mul = kv_mul; a.head_size = head_size; a.seg_cap = wa.seg_cap;
    if (x3 != nullptr && (kp & 3) == 0 && (((uintptr_t)x3) & 7) == 0) { a.x3 = (__bf16 *)x3; a.kp = kp; }
    const int mq = kv_mul == 1 ? 1 : kv_mul == 2 ? 2 : kWaHeadsMax;
    const dim3 grid(n_heads / kv_mul * ((kv_mul + mq - 1) / mq), wa.n_seg, n);
    switch (mq) {
        case 1: hipLaunchKernelGGL(wide_attention<1>, grid, dim3(kWaBlock), 0, st, a); break;
        case 2: hipLaunchKernelGGL(wide_attention<2>, grid, dim3(kWaBlock), 0, st, a); break;
        default: hipLaunchKernelGGL(wide_attention<kWaHeadsMax>, grid, dim3(kWaBlock), 0, st, a); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wide_combine, dim3(n_heads, n), dim3(64), 0, st, a);
    e = hipGetLastError();
    if (e == hipSuccess && planes_written) *planes_written = a.x3 != nullptr;
    return e;
}

hipError_t launch_wide_logits_out(const float *logits, int ld, const WideTable *tab, int vocab, int *next, int n, hipStream_t st)
{
    if (n < 1 || n > kWideMax || vocab < 1 || ld < vocab || logits == nullptr || tab == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_logits_out, dim3(n), dim3(1024), 0, st, logits, ld, tab, vocab, next);
    return hipGetLastError();
}

}  // namespace l2z
