// wide_decode.hip -- the kernels l2z_transformer_wide adds to the ragged prompt pass (wide_decode.h; host side:
// wide_host.cpp): decode attention for many one-query sequences, each on its own cache, split over positions in the verify
// family's fixed segments of absolute positions, and the launch that hands the logits matrix back to the runstates.
//
// The attention is the verify family's segment body (verify_device.h) with a block's query slots being the query heads
// of one kv head of ONE row, so the summation orders are that file's.  A row's results depend on that row's q, its own
// cache rows 0 .. pos and its own position only: no block touches two sequences.  Vector loads and stores only; every
// FMA is an explicit fmaf.
#include "wide_decode.h"

#include "kernel_common.h"
#include "prefill_common.h"
#include "verify_device.h"

namespace l2z {
namespace {

constexpr int kWcUB = 4;        // combine: segments' partials a lane has in flight
constexpr int kWaHeadsMax = 4;  // query heads of one kv head a block serves (8: 256 VGPRs, one wave per SIMD)

struct WideAttnArgs {
    const float *q;
    float *out;
    const int32_t *pos;       // [rows of the chunk] a row's position
    const RaggedSeq *seq;     // [sequence slots] the caches (and pages) of a slot
    const int2 *list;         // != null (l2z_step_mixed): block ordinal i serves row list[i].x of sequence slot list[i].y;
                              // null: row = slot = ordinal
    float *part_o, *part_ml;  // [kWideMax, n_heads, seg_cap, head_size] and [..., 2], by ORDINAL
    size_t layer_off, kv_head_stride;
    size_t page_floats;       // paged sequences (RaggedSeq::pages): floats per page of the pool
    int ldq, ldo, n_heads, kv_mul, head_size, seg_cap;
    __bf16 *x3;  // != null: out's planes of bf16 terms too
    int kp;
};

// Block (kv head x part, segment, ordinal); MQ = query heads per block (a part = MQ consecutive heads of the kv head: one part
// while kv_mul <= kWaHeadsMax).  The part's heads are the slots of segment_attention_body: every head sees the keys up to
// the row's position, which is where the segment ends for the block.
template <int MQ>
__global__ __launch_bounds__(kVaBlock) void wide_attention(const WideAttnArgs a)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<MQ>];
    const int ord = blockIdx.z, seg = blockIdx.y;
    int row = ord, slot = ord;
    if (a.list != nullptr) { const int2 d = a.list[ord]; row = d.x; slot = d.y; }   // (uniform)
    const int pos = a.pos[row];
    const int seg0 = seg * kVerifySeg;
    if (seg0 > pos) return;  // past this row's last segment (uniform, before any barrier)
    const int parts = (a.kv_mul + MQ - 1) / MQ;
    const int kvh = blockIdx.x / parts, hq0 = (blockIdx.x % parts) * MQ;
    const int h0 = kvh * a.kv_mul + hq0;
    const int nq = min(MQ, a.kv_mul - hq0);
    SegSlots s = {};
    s.q = a.q + (size_t)row * a.ldq + (size_t)h0 * a.head_size; s.q_step = (size_t)a.head_size;
    s.see0 = pos; s.see_step = 0;
    s.idx0 = (size_t)ord * a.n_heads + h0; s.part_step = 1;
    s.act = (1u << nq) - 1u;
    s.part_o = a.part_o; s.part_ml = a.part_ml; s.seg_cap = a.seg_cap;
    const RaggedSeq sq = a.seq[slot];
    size_t head_off = a.layer_off + (size_t)kvh * a.kv_head_stride;
    // paged: the block's segment is ONE page; the body addresses key t at base + t * head_size, so the base takes the
    // page's start less the segment's first row (one dependent 4-byte read per block, uniform)
    if (sq.pages != nullptr) head_off += (size_t)kv_page_id(sq.pages, seg) * a.page_floats - (size_t)seg0 * a.head_size;
    segment_attention_body<MQ>(s, sq.kc + head_off, sq.vc + head_off, a.head_size, seg, min(seg0 + kVerifySeg - 1, pos), sc);
}

// Block (head, ordinal), lane c = four features: the row's segments 0 .. pos / kVerifySeg through segment_combine_body
__global__ __launch_bounds__(64) void wide_combine(const WideAttnArgs a)
{
    const int h = blockIdx.x, ord = blockIdx.y, c = threadIdx.x, hs = a.head_size;
    if (c >= (hs >> 2)) return;
    const int row = a.list != nullptr ? a.list[ord].x : ord;
    const v4f r = segment_combine_body<kWcUB>(a.part_o, a.part_ml, ((size_t)ord * a.n_heads + h) * a.seg_cap,
                                              a.pos[row] / kVerifySeg + 1, hs, c);
    *(v4f *)(a.out + (size_t)row * a.ldo + (size_t)h * hs + 4 * c) = r;
    if (a.x3) planes_store4(a.x3, a.kp, row, h * hs + 4 * c, r);
}

// Block = row, 1024 threads: the copy, and the argmax of what was copied.  A thread takes its elements in increasing
// index order (strict '>' keeps the lowest index of equal values; a NaN counts only as element 0); the candidates
// combine by argmax_merge (value, then lower index; the NaN at index 0 above all): argmax_rule.h, NaN rows included.
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
        next[row] = argmax_token(cand);
    }
}

}  // namespace

// what the launchers ask of the partials and the output, and the arguments the combine reads
static bool wide_out_args(WideAttnArgs &a, float *out, int ldo, const WideRows &wr, int n_heads, int head_size, void *x3, int kp)
{
    if (wr.n < 1 || wr.n > kWideMax || head_size < 4 || head_size > 256 || (head_size & 3) || n_heads < 1 || wr.pos == nullptr ||
        wr.seq == nullptr || wr.part == nullptr || wr.n_seg < 1 || wr.n_seg > wr.seg_cap || (ldo & 3) ||
        (((uintptr_t)out | (uintptr_t)wr.part) & 15))
        return false;
    a.out = out; a.pos = wr.pos; a.seq = wr.seq; a.list = wr.list;
    a.part_o = wr.part;
    a.part_ml = wr.part + (size_t)kWideMax * n_heads * wr.seg_cap * head_size;
    a.ldo = ldo; a.n_heads = n_heads; a.head_size = head_size; a.seg_cap = wr.seg_cap;
    if (x3 != nullptr && (kp & 3) == 0 && (((uintptr_t)x3) & 7) == 0) { a.x3 = (__bf16 *)x3; a.kp = kp; }
    return true;
}

// the wide step's rows: row i of the chunk = sequence slot i of the table
static WideRows rows_of(const WideAttn &wa, int n)
{
    WideRows wr = {};
    if (wa.tab != nullptr) { wr.pos = wa.tab->pos; wr.seq = wa.tab->seq; }
    wr.n = n; wr.part = wa.part; wr.seg_cap = wa.seg_cap; wr.n_seg = wa.n_seg; wr.page_floats = wa.page_floats;
    return wr;
}

static hipError_t combine_launch(const WideAttnArgs &a, int n, hipStream_t st, bool *planes_written)
{
    hipLaunchKernelGGL(wide_combine, dim3(a.n_heads, n), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess && planes_written) *planes_written = a.x3 != nullptr;
    return e;
}

hipError_t launch_wide_attention_rows(const RaggedLayer &L, const WideRows &wr, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    const int kv_mul = L.kv_mul;
    WideAttnArgs a = {};
    if (!wide_out_args(a, L.out, L.ldo, wr, L.n_heads, L.head_size, L.x3, L.kp) || kv_mul < 1 || L.n_heads % kv_mul != 0 || (L.ldq & 3) ||
        (((uintptr_t)L.q) & 15) || (L.layer_off & 3) || (L.kv_head_stride & 3) || (wr.page_floats & 3))
        return hipErrorInvalidValue;
    a.q = L.q; a.ldq = L.ldq; a.kv_mul = kv_mul;
    a.layer_off = L.layer_off; a.kv_head_stride = L.kv_head_stride; a.page_floats = wr.page_floats;
    const int mq = kv_mul == 1 ? 1 : kv_mul == 2 ? 2 : kWaHeadsMax;
    const dim3 grid(L.n_heads / kv_mul * ((kv_mul + mq - 1) / mq), wr.n_seg, wr.n);
    switch (mq) {
        case 1: hipLaunchKernelGGL(wide_attention<1>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 2: hipLaunchKernelGGL(wide_attention<2>, grid, dim3(kVaBlock), 0, L.st, a); break;
        default: hipLaunchKernelGGL(wide_attention<kWaHeadsMax>, grid, dim3(kVaBlock), 0, L.st, a); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return combine_launch(a, wr.n, L.st, planes_written);
}

hipError_t launch_wide_attention(const RaggedLayer &L, const WideAttn &wa, bool *planes_written)
{
    return launch_wide_attention_rows(L, rows_of(wa, L.P), planes_written);
}

hipError_t launch_wide_combine(float *out, int ldo, const WideAttn &wa, int n, int n_heads, int head_size, hipStream_t st,
                               void *x3, int kp, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    WideAttnArgs a = {};
    if (!wide_out_args(a, out, ldo, rows_of(wa, n), n_heads, head_size, x3, kp)) return hipErrorInvalidValue;
    return combine_launch(a, n, st, planes_written);
}

hipError_t launch_wide_logits_out(const float *logits, int ld, const WideTable *tab, int vocab, int *next, int n, hipStream_t st)
{
    if (n < 1 || n > kWideMax || vocab < 1 || ld < vocab || logits == nullptr || tab == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_logits_out, dim3(n), dim3(1024), 0, st, logits, ld, tab, vocab, next);
    return hipGetLastError();
}

}  // namespace l2z
