// q8_matvec.hip -- the decode's row mat-vec on int8 group-quantized weights (llama2.c version-2 checkpoints, DESIGN.md
// 4.23), its launcher, and the group quantization as launches of its own (the weights of l2z_weights_init_q8_from,
// l2z_q8_quantize).  Compiled with -ffp-contract=off like every kernel file.
//
//   out[i] = sum over groups g of  f32(I[i][g]) * ws[i][g] * xs[g],   I[i][g] = sum over the group of wq * xq   (int32, exact)
//
// Prologue, repeated by every block as the f32 kernels repeat their rmsnorm: x is read from memory (twice where the
// launch has a norm: the sum of squares first), normalised, quantized per group by the activation rule -- four values a
// thread, the group's maximum taken across the 8 or 16 lanes that hold it -- and kept in LDS as n / 4 packed dwords and
// n / gs scales.  Wo and W2 take it without the norm; l2z_q8_matmul brings an x quantized already.
//
// A wave owns a pair of rows (rows 2p, 2p + 1 of the concatenated row space, or row p of W1 and of W3: matvec_device.h's
// pairs, so its epilogues run unchanged).  Lane l of step k loads the 16 bytes at l + 64 k of either row: 1 KiB a load
// instruction, contiguous across the wave, and the four waves of a block sweep four adjacent pairs; a wave requests its
// first batch before the block stages x and the next batch -- the next pair's first included -- before it reduces.  A lane's 16 values
// lie inside one group; four v_dot4c_i32_i8 against the matching 16 bytes of x in LDS give its int32 partial, the 2
// (gs 32) or 4 (gs 64) lanes of a group add theirs across lanes, and the group's first lane scales the sum --
// (f32(I) * ws) * xs, runq.c's order -- into its f32 accumulator.  A wave-wide sum ends the row.  Which lane takes which
// group, and the order of the sums, are functions of n and gs only: the same bits from run to run, whatever the grid.
#include "argmax_rule.h"
#include "matvec_device.h"
#include "q8_device.h"

namespace l2z {
namespace {

constexpr int kQ8U = 4;  // 16-byte loads per row per lane in flight

// x -> LDS: xq [n / 4] packed dwords, xsc [n / GS] scales
template <int GS>
__device__ __forceinline__ void q8_stage_x(const Q8MatvecArgs &a, int n, int *xq, float *xsc, float *scratch)
{
    constexpr int L4 = GS / 4;  // lanes that hold a group here
    const int tid = threadIdx.x, n4 = n >> 2;
    if (a.xq != nullptr) {
        const int *src = (const int *)a.xq;
        for (int j = tid; j < n4; j += kBlock) xq[j] = src[j];
        for (int j = tid; j < n / GS; j += kBlock) xsc[j] = a.xs[j];
        __syncthreads();
        return;
    }
    const v4f *x4 = (const v4f *)a.b.x, *g4 = (const v4f *)a.b.rms_w;
    const bool norm = a.b.rms_w != nullptr;
    float s = 1.0f;
    if (norm) {  // main.zig:432-468, the arithmetic of kernel_common.h's staging
        float ss = 0.0f;
        for (int j = tid; j < n4; j += kBlock) {
            const v4f v = x4[j];
            ss = fmaf(v.x, v.x, ss);
            ss = fmaf(v.y, v.y, ss);
            ss = fmaf(v.z, v.z, ss);
            ss = fmaf(v.w, v.w, ss);
        }
        const float tot = block_sum(ss, scratch);
        s = tot / (float)n;
        s += 1e-5f;
        s = 1.0f / sqrtf(s);
    }
    // n4 is a multiple of L4 and L4 divides 64: the lanes of a group are all in the loop together
    for (int j = tid; j < n4; j += kBlock) {
        v4f v = x4[j];
        if (norm) {
            const v4f g = g4[j];
            v.x = (v.x * s) * g.x;
            v.y = (v.y * s) * g.y;
            v.z = (v.z * s) * g.z;
            v.w = (v.w * s) * g.w;
        }
        float sc;
        xq[j] = q8_quant4<GS, false>(v, &sc);
        if ((tid % L4) == 0) xsc[j / L4] = sc;
    }
    __syncthreads();
}

// the two rows of pair p: their values and their scales
template <int EPI>
__device__ __forceinline__ void q8_pair_rows(const Q8MatvecArgs &a, const MvLocals &m, int p, int ng, const int8_t *&qa,
                                             const int8_t *&qb, const float *&sa, const float *&sb)
{
    if (EPI == EPI_SWIGLU) {  // W1 | W3 row-interleaved
        qa = a.q0 + (size_t)(2 * p) * (size_t)m.n;
        qb = qa + m.n;
        sa = a.s0 + (size_t)(2 * p) * (size_t)ng;
        sb = sa + ng;
        return;
    }
    const int ga = 2 * p;
    const int gb = (ga + 1 < m.total_rows) ? ga + 1 : ga;
    const SegRow ra = seg_row(m, ga), rb = seg_row(m, gb);
    qa = ra.pick(a.q0, a.q1, a.q2) + (size_t)ra.row * (size_t)m.n;
    qb = rb.pick(a.q0, a.q1, a.q2) + (size_t)rb.row * (size_t)m.n;
    sa = ra.pick(a.s0, a.s1, a.s2) + (size_t)ra.row * (size_t)ng;
    sb = rb.pick(a.s0, a.s1, a.s2) + (size_t)rb.row * (size_t)ng;
}

__device__ __forceinline__ int q8_dot16(v4i w, v4i x)
{
    int acc = __builtin_amdgcn_sdot4(w.x, x.x, 0, false);
    acc = __builtin_amdgcn_sdot4(w.y, x.y, acc, false);
    acc = __builtin_amdgcn_sdot4(w.z, x.z, acc, false);
    return __builtin_amdgcn_sdot4(w.w, x.w, acc, false);
}

template <int EPI, int GS>
__global__ __launch_bounds__(kBlock) void q8_matvec_kernel(const Q8MatvecArgs a)
{
    constexpr int LPG = GS / 16;  // lanes that share a group in the product
    constexpr int U = kQ8U;
    extern __shared__ __attribute__((aligned(16))) int q8_lds[];
    const MvLocals m = mv_locals<EPI>(a.b);  // (the launcher leaves b.push null: q8 weights are unsharded)
    const int n = m.n, nch = n >> 4, ng = n / GS;
    int *xq = q8_lds;
    float *xsc = (float *)(q8_lds + (n >> 2));
    float *scratch = xsc + ng;
    const v4i *xq4 = (const v4i *)xq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool leader = (lane % LPG) == 0;
    const int ustride = gridDim.x * kWaves;
    int u = blockIdx.x * kWaves + wave;
    const bool has_unit = u < m.n_pairs;

    // the registers of one batch: U chunks of either row of the pair, and their groups' scales
    const int8_t *qa, *qb;
    const float *wsa, *wsb;
    v4i wa[U], wb[U];
    float fa[U], fb[U];
    auto load = [&](int c0) __attribute__((always_inline)) {
        const v4i *a4 = (const v4i *)qa, *b4 = (const v4i *)qb;
#pragma unroll
        for (int k = 0; k < U; k++) {  // chunks past the row end load nothing: their products are zero
            const int c = c0 + kWave * k;
            const bool in_row = c < nch;
            wa[k] = in_row ? __builtin_nontemporal_load(a4 + c) : v4i{0, 0, 0, 0};
            wb[k] = in_row ? __builtin_nontemporal_load(b4 + c) : v4i{0, 0, 0, 0};
            fa[k] = in_row ? wsa[c / LPG] : 0.0f;
            fb[k] = in_row ? wsb[c / LPG] : 0.0f;
        }
    };
    // the first batch is requested BEFORE the block stages x, like the f32 kernels': the weights travel while x is
    // normalised and quantized
    q8_pair_rows<EPI>(a, m, has_unit ? u : 0, ng, qa, qb, wsa, wsb);
    EpiIn ein = epi_prefetch<EPI>(m, has_unit ? u : 0, lane == 0 && has_unit);
    EpiIn ein_next = ein;
    if (has_unit) load(lane);
    q8_stage_x<GS>(a, n, xq, xsc, scratch);

    // flat loop over (unit, batch): consume the batch in the registers, request the next one -- the next unit's first
    // included -- and only then reduce and store
    ArgmaxCand best;  // EPI_ARGMAX: running (max, first index) of this wave's rows
    float acc_a = 0.0f, acc_b = 0.0f;
    int c0 = lane;
    bool more = has_unit;
    while (more) {
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int c = c0 + kWave * k;
            const bool in_row = c < nch;
            const int cc = in_row ? c : 0;
            const v4i xv = xq4[cc];
            // nch is a multiple of LPG: a group's lanes are in the row together; the sum across them runs on all lanes
            const int ia = q8_lanes_sum<LPG>(q8_dot16(wa[k], xv));
            const int ib = q8_lanes_sum<LPG>(q8_dot16(wb[k], xv));
            if (leader && in_row) {
                const float xs = xsc[cc / LPG];
                acc_a += ((float)ia * fa[k]) * xs;
                acc_b += ((float)ib * fb[k]) * xs;
            }
        }
        const bool unit_done = c0 - lane + kWave * U >= nch;  // (wave-uniform)
        const int u_next = unit_done ? u + ustride : u;
        const int c0_next = unit_done ? lane : c0 + kWave * U;
        more = u_next < m.n_pairs;
        if (more) {
            if (unit_done) {
                q8_pair_rows<EPI>(a, m, u_next, ng, qa, qb, wsa, wsb);
                ein_next = epi_prefetch<EPI>(m, u_next, lane == 0);
            }
            load(c0_next);
        }
        if (unit_done) {
            const float sa = wave_sum(acc_a), sb = wave_sum(acc_b);
            pair_epilogue<EPI>(m, u, sa, sb, lane == 0, ein);
            if (EPI == EPI_ARGMAX) {  // single segment: pair u = rows 2u, 2u + 1, taken in increasing order
                const int ra_ = 2 * u, rb_ = ra_ + 1;
                argmax_take(best, sa, ra_ + a.b.row_offset);
                if (rb_ < m.total_rows) argmax_take(best, sb, rb_ + a.b.row_offset);
            }
            ein = ein_next;
            acc_a = 0.0f;
            acc_b = 0.0f;
        }
        u = u_next;
        c0 = c0_next;
    }
    if (EPI == EPI_ARGMAX) {
        // block candidate, as matvec_kernel's: larger value wins, equal values -> lower index (argmax_rule.h)
        argmax_wave_fold(best);
        __syncthreads();
        if (lane == 0) {
            scratch[wave] = best.v;
            scratch[kWaves + wave] = __int_as_float(best.i);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            ArgmaxCand c = {scratch[0], __float_as_int(scratch[kWaves])};
            for (int w = 1; w < kWaves; w++) argmax_merge(c, scratch[w], __float_as_int(scratch[kWaves + w]));
            a.b.part_val[blockIdx.x] = c.v;
            a.b.part_idx[blockIdx.x] = c.i;
        }
    }
}

// count / 4 float4 of src -> packed dwords and one scale per group
template <int GS, bool EVEN>
__global__ __launch_bounds__(kBlock) void q8_quantize_kernel(const float *__restrict__ src, size_t n4, bool vec, int *q, float *s)
{
    constexpr int L4 = GS / 4;
    const size_t stride = (size_t)gridDim.x * kBlock;
    // n4 is a multiple of L4, the stride of 64: the lanes of a group are all in the loop together
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < n4; j += stride) {
        v4f v;
        if (vec) v = ((const v4f *)src)[j];
        else v = v4f{src[4 * j], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]};
        float sc;
        q[j] = q8_quant4<GS, EVEN>(v, &sc);
        if ((threadIdx.x % L4) == 0) s[j / L4] = sc;
    }
}

template <int GS>
const void *q8_pick(int epi)
{
    switch (epi) {
        case EPI_STORE: return reinterpret_cast<const void *>(&q8_matvec_kernel<EPI_STORE, GS>);
        case EPI_ROPE: return reinterpret_cast<const void *>(&q8_matvec_kernel<EPI_ROPE, GS>);
        case EPI_RESID: return reinterpret_cast<const void *>(&q8_matvec_kernel<EPI_RESID, GS>);
        case EPI_SWIGLU: return reinterpret_cast<const void *>(&q8_matvec_kernel<EPI_SWIGLU, GS>);
        case EPI_ARGMAX: return reinterpret_cast<const void *>(&q8_matvec_kernel<EPI_ARGMAX, GS>);
        default: return nullptr;
    }
}

}  // namespace

hipError_t launch_q8_matvec(const Q8MatvecArgs &a_in, int epi, int max_blocks_per_cu, int n_cus, hipStream_t st, int *out_grid)
{
    Q8MatvecArgs a = a_in;
    a.b.push = nullptr;
    a.b.xin = LLIn{};
    const int n = a.b.n, gs = a.gs;
    if ((gs != 32 && gs != 64) || n <= 0 || n % gs != 0) return hipErrorInvalidValue;
    if (epi == EPI_SWIGLU && a.b.rows1 != a.b.rows0) return hipErrorInvalidValue;
    if (epi == EPI_ARGMAX && (a.b.rows1 != 0 || a.b.rows2 != 0 || a.b.part_val == nullptr || a.b.part_idx == nullptr))
        return hipErrorInvalidValue;
    const int total_rows = a.b.rows0 + a.b.rows1 + a.b.rows2;
    const int n_pairs = epi == EPI_SWIGLU ? a.b.rows0 : (total_rows + 1) / 2;
    if (n_pairs <= 0 || a.q0 == nullptr || a.s0 == nullptr) return hipErrorInvalidValue;
    if ((a.b.rows1 > 0 && epi != EPI_SWIGLU && (a.q1 == nullptr || a.s1 == nullptr)) ||
        (a.b.rows2 > 0 && (a.q2 == nullptr || a.s2 == nullptr)))
        return hipErrorInvalidValue;
    // 16-byte loads of the rows (n is a multiple of 32) and of x; dword reads of a quantized x
    if (!aligned16(a.q0) || (a.q1 != nullptr && !aligned16(a.q1)) || (a.q2 != nullptr && !aligned16(a.q2))) return hipErrorInvalidValue;
    if (a.xq != nullptr ? (a.xs == nullptr || ((uintptr_t)a.xq & 3u) != 0) : !aligned16(a.b.x)) return hipErrorInvalidValue;
    if (a.xq == nullptr && a.b.rms_w != nullptr && !aligned16(a.b.rms_w)) return hipErrorInvalidValue;
    const void *fn = gs == 32 ? q8_pick<32>(epi) : q8_pick<64>(epi);
    if (fn == nullptr) return hipErrorInvalidValue;
    const size_t lds = (size_t)n + (size_t)(n / gs + kScratch) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // Grid (matvec_device.h): at most what is resident at once, pairs dealt round-robin to the waves
    if (max_blocks_per_cu < 1 || max_blocks_per_cu > 8) max_blocks_per_cu = 8;  // (matvec_max_grid: the candidates' room)
    const int grid = mv_grid_wave_units(n_pairs, mv_resident_blocks(fn, lds, max_blocks_per_cu, n_cus, 0));
    if (out_grid) *out_grid = grid;
    void *args[] = {&a};
    return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, lds, st);
}

hipError_t launch_q8_quantize(const float *src, size_t count, int gs, bool weight_rule, int8_t *q, float *s, hipStream_t st)
{
    if ((gs != 32 && gs != 64) || count == 0 || count % (size_t)gs != 0 || ((uintptr_t)q & 3u) != 0) return hipErrorInvalidValue;
    const size_t n4 = count / 4;
    const size_t blocks = (n4 + kBlock - 1) / kBlock;
    const int grid = (int)(blocks < 16384 ? blocks : 16384);
    const bool vec = aligned16(src);
    const void *fn = gs == 32 ? (weight_rule ? (const void *)&q8_quantize_kernel<32, true> : (const void *)&q8_quantize_kernel<32, false>)
                              : (weight_rule ? (const void *)&q8_quantize_kernel<64, true> : (const void *)&q8_quantize_kernel<64, false>);
    int *qd = (int *)q;
    size_t n4_ = n4;
    bool vec_ = vec;
    void *args[] = {&src, &n4_, &vec_, &qd, &s};
    return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, 0, st);
}

}  // namespace l2z
