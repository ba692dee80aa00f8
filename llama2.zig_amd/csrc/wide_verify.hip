// wide_verify.hip -- the kernels l2z_verify_wide adds to the wide step (wide_decode.h; host side: wide_host.cpp): causal
// attention for up to kWideMax rows that belong to SEVERAL sequences of up to kBatchMax consecutive positions each, and the
// verdict per sequence.
//
// The attention is the verify family's segment body (verify_device.h) with a block's query slots being the rows of ONE
// sequence at one head, set up as verify_attention_body sets them up; the q slices and the partials are the wide step's,
// indexed by the row's place in the chunk, so wide_combine (wide_decode.hip) folds them as it stands.  A row's results
// depend on its own sequence's q rows up to itself, that sequence's cache rows and its position only: no block touches two
// sequences.  The verdict draws every row's token with the sampler's row body (sample_device.h) and scans each sequence's
// own rows.  Vector loads and stores only; every FMA is an explicit fmaf.
#include "wide_decode.h"

#include "kernel_common.h"
#include "sample_device.h"
#include "verify_device.h"

namespace l2z {
namespace {

struct WideVerifyAttnArgs {
    const float *q;
    const WideTable *tab;
    float *part_o, *part_ml;  // [kWideMax, n_heads, seg_cap, head_size] and [..., 2]
    size_t layer_off, kv_head_stride;
    size_t page_floats;       // paged sequences (RaggedSeq::pages): floats per page of the pool
    int ldq, n_heads, kv_mul, head_size, seg_cap;
};

// Block (head, segment, sequence); M >= the sequence's rows.  Slot i is row row0 + i of the chunk: it sees the keys up to
// pos0 + i, and is in use when it is a row of the sequence that reaches this segment (i >= i0).
template <int M>
__global__ __launch_bounds__(kVaBlock) void wide_verify_attention(const WideVerifyAttnArgs a)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<M>];
    const int h = blockIdx.x, seg = blockIdx.y;
    const RaggedSeq sq = a.tab->seq[blockIdx.z];
    const int seg0 = seg * kVerifySeg;
    if (seg0 > sq.pos0 + sq.rows - 1) return;  // past this sequence's last segment (uniform, before any barrier)
    const int last = min(seg0 + kVerifySeg, sq.pos0 + sq.rows) - 1;  // the last key of this segment any row sees
    const int i0 = max(0, seg0 - sq.pos0);                           // rows below i0 end before this segment (i0 < rows)
    SegSlots s = {};
    s.q = a.q + (size_t)sq.row0 * a.ldq + (size_t)h * a.head_size; s.q_step = (size_t)a.ldq;
    s.see0 = sq.pos0; s.see_step = 1;
    s.idx0 = (size_t)sq.row0 * a.n_heads + h; s.part_step = (size_t)a.n_heads;
    s.act = ((1u << sq.rows) - 1u) & (0xFFFFFFFFu << i0);
    s.part_o = a.part_o; s.part_ml = a.part_ml; s.seg_cap = a.seg_cap;
    size_t head_off = a.layer_off + (size_t)(h / a.kv_mul) * a.kv_head_stride;
    // paged: the segment is ONE page, the base takes its start less the segment's first row (as wide_attention)
    if (sq.pages != nullptr) head_off += (size_t)kv_page_id(sq.pages, seg) * a.page_floats - (size_t)seg0 * a.head_size;
    segment_attention_body<M>(s, sq.kc + head_off, sq.vc + head_off, a.head_size, seg, last, sc);
}

// Block = row, 1024 threads: wide_draw_advance's draw without the hand-over
__global__ __launch_bounds__(kSbThreads) void wide_verify_draw(const WideVerdict a)
{
    __shared__ SampleLds L;
    const int row = blockIdx.x;
    const int j = a.tab->row_seq[row];
    const float temperature = a.ctl ? a.ctl->temperature[j] : 0.0f;
    const bool greedy = temperature == 0.0f;
    int next = sample_row(L, a.logits + (size_t)row * a.ld, a.vocab, temperature, greedy ? 0.0f : a.ctl->top_p[j],
                          greedy ? 0.0f : a.ctl->coins[row], greedy ? nullptr : a.scratch + (size_t)row * a.row_stride);
    if (threadIdx.x == 0) {
        // Unreachable by construction (sample_row returns an index it scanned or a candidate's id); kept as
        // wide_draw_advance keeps its own
        if ((unsigned)next >= (unsigned)a.vocab) next = 0;
        a.next[row] = next;
    }
}

// Block = sequence, 1024 threads: verify_batch_accept_kernel's scan over the sequence's own rows (at most 15 compares),
// then row row0 + a of the matrix -> the sequence's runstate, wide_logits_out's copy
__global__ __launch_bounds__(1024) void wide_verify_accept(const WideVerdict a)
{
    __shared__ int s_a;
    const int j = blockIdx.x, tid = threadIdx.x;
    const int first = a.tab->seq[j].row0, n = a.tab->seq[j].rows;
    if (tid == 0) {
        int acc = 0;
        while (acc + 1 < n && a.tab->tokens[first + acc + 1] == a.next[first + acc]) acc++;
        s_a = acc;
        a.accepted[j] = acc;
    }
    __syncthreads();
    block_copy_row(a.tab->logits[j], a.logits + (size_t)(first + s_a) * a.ld, a.vocab, tid, 1024);
}

}  // namespace

hipError_t launch_wide_verify_attention(const RaggedLayer &L, const WideAttn &wa, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    const int n_seq = wa.n_seq, n_rows = L.P, n_heads = L.n_heads, head_size = L.head_size, kv_mul = L.kv_mul;
    if (n_seq < 1 || n_seq > n_rows || n_rows > kWideMax || head_size < 4 || head_size > 256 || (head_size & 3) || kv_mul < 1 ||
        n_heads < 1 || n_heads % kv_mul != 0 || wa.tab == nullptr || wa.part == nullptr || wa.n_seg < 1 || wa.n_seg > wa.seg_cap ||
        (L.ldq & 3) || (((uintptr_t)L.q | (uintptr_t)wa.part) & 15) || (L.layer_off & 3) || (L.kv_head_stride & 3) ||
        (wa.page_floats & 3))
        return hipErrorInvalidValue;
    WideVerifyAttnArgs a = {};
    a.q = L.q; a.tab = wa.tab;
    a.part_o = wa.part;
    a.part_ml = wa.part + (size_t)kWideMax * n_heads * wa.seg_cap * head_size;
    a.layer_off = L.layer_off; a.kv_head_stride = L.kv_head_stride; a.page_floats = wa.page_floats;
    a.ldq = L.ldq; a.n_heads = n_heads; a.kv_mul = kv_mul; a.head_size = head_size; a.seg_cap = wa.seg_cap;
    const dim3 grid(n_heads, wa.n_seg, n_seq);
    switch (wa.verify_m) {
        case 1: hipLaunchKernelGGL(wide_verify_attention<1>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 2: hipLaunchKernelGGL(wide_verify_attention<2>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 4: hipLaunchKernelGGL(wide_verify_attention<4>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 8: hipLaunchKernelGGL(wide_verify_attention<8>, grid, dim3(kVaBlock), 0, L.st, a); break;
        case 16: hipLaunchKernelGGL(wide_verify_attention<16>, grid, dim3(kVaBlock), 0, L.st, a); break;
        default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_wide_combine(L.out, L.ldo, wa, n_rows, n_heads, head_size, L.st, L.x3, L.kp, planes_written);
}

hipError_t launch_wide_verdict(const WideVerdict &d, int n_seq, int n_rows, hipStream_t st)
{
    if (n_seq < 1 || n_seq > n_rows || n_rows > kWideMax || d.vocab < 1 || d.ld < d.vocab || d.logits == nullptr ||
        d.tab == nullptr || d.next == nullptr || d.accepted == nullptr)
        return hipErrorInvalidValue;
    if (d.ctl != nullptr && (d.scratch == nullptr || d.row_stride < sample_scratch_floats(d.vocab))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_verify_draw, dim3(n_rows), dim3(kSbThreads), 0, st, d);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wide_verify_accept, dim3(n_seq), dim3(1024), 0, st, d);
    return hipGetLastError();
}

}  // namespace l2z
