// mixed_step.hip -- what l2z_step_mixed adds to the ragged prompt pass (mixed_step.h; host side: wide_host.cpp): the
// attention dispatch of a chunk in which only SOME rows are one-row sequences, and the call's last launch.
//
// The dispatch launches no kernel of its own.  The sequences of several rows go through launch_ragged_attention
// (prefill_ragged.hip); the one-row sequences through launch_wide_attention_rows (wide_decode.hip): wide_attention and
// wide_combine with the table's decode list, whose entry names the row in the chunk (q, out, the planes) and the sequence
// slot (caches, pages), the partials standing at the entry's ordinal -- so the wide step's allocation of kWideMax rows holds
// them whatever the chunk's row count.  With every sequence of one row the list is the identity and every address, every sum
// and every bit is the wide step's.  Vector loads and stores only; every FMA is an explicit fmaf.
#include "mixed_step.h"

#include "kernel_common.h"
#include "sample_device.h"
#include "wide_decode.h"

namespace l2z {
namespace {

// Block = sequence, 1024 threads: the draw from the sequence's row of the compact matrix, then that row -> the runstate
// (wide_logits_out's copy)
__global__ __launch_bounds__(kSbThreads) void mixed_draw_out(const MixedDraw a)
{
    __shared__ SampleLds L;
    const int j = blockIdx.x, tid = threadIdx.x;
    const float *src = a.logits + (size_t)j * a.ld;
    const float temperature = a.sampled ? a.tab->temperature[j] : 0.0f;
    const bool greedy = temperature == 0.0f;
    int next = sample_row(L, src, a.vocab, temperature, greedy ? 0.0f : a.tab->top_p[j], greedy ? 0.0f : a.tab->coins[j],
                          greedy ? nullptr : a.scratch + (size_t)j * a.row_stride);
    if (tid == 0) {
        // Unreachable by construction (sample_row returns an index it scanned or a candidate's id); kept as
        // wide_verify_draw keeps its own
        if ((unsigned)next >= (unsigned)a.vocab) next = 0;
        a.next[j] = next;
    }
    block_copy_row(a.tab->logits[j], src, a.vocab, tid, kSbThreads);
}

}  // namespace

hipError_t launch_mixed_attention(const RaggedLayer &L, const MixedAttn &m, const RaggedChunk &rg, bool *planes_written)
{
    if (planes_written) *planes_written = false;
    const int head_size = L.head_size;
    if (L.P < 1 || L.P > kMixedRowsMax || m.n_dec < 0 || m.n_dec > kMixedSeqMax || m.n_prompt_rows < 0 || m.n_dec + m.n_prompt_rows != L.P ||
        head_size < 4 || head_size > 256 || (head_size & 3) || L.n_heads < 1 || L.kv_mul < 1 || L.n_heads % L.kv_mul != 0 ||
        m.tab == nullptr || (L.ldq & 3) || (L.ldo & 3) || (((uintptr_t)L.q | (uintptr_t)L.out) & 15) || (L.layer_off & 3) ||
        (L.kv_head_stride & 3) || (m.page_floats & 3))
        return hipErrorInvalidValue;
    if (m.n_dec > 0 && (m.part == nullptr || (((uintptr_t)m.part) & 15) || m.n_seg < 1 || m.n_seg > m.seg_cap))
        return hipErrorInvalidValue;
    // The planes of out: the flash form writes its rows' (launch_ragged_attention), the block-per-(head, row) form does not --
    // so with rows of several-row sequences at another head size NEITHER class writes them and the chunk splits out itself.
    const bool flash = head_size == 64 || head_size == 128;
    const bool planes = L.x3 != nullptr && (L.kp & 3) == 0 && (((uintptr_t)L.x3) & 7) == 0 && (flash || m.n_prompt_rows == 0);
    RaggedLayer each = L;   // both classes' launches: with the planes, or without
    if (!planes) each.x3 = nullptr;
    if (m.n_prompt_rows > 0) {
        bool pw = false;
        const hipError_t e = launch_ragged_attention(each, rg, &pw);
        if (e != hipSuccess) return e;
        if (pw != planes) return hipErrorInvalidValue;   // (never a mixture)
    }
    if (m.n_dec > 0) {
        WideRows wr = {};
        wr.pos = m.tab->pos; wr.seq = m.tab->seq; wr.list = m.tab->dec;
        wr.n = m.n_dec; wr.part = m.part; wr.seg_cap = m.seg_cap; wr.n_seg = m.n_seg; wr.page_floats = m.page_floats;
        bool pw = false;
        const hipError_t e = launch_wide_attention_rows(each, wr, &pw);
        if (e != hipSuccess) return e;
        if (pw != planes) return hipErrorInvalidValue;
    }
    if (planes_written) *planes_written = planes;
    return hipSuccess;
}

hipError_t launch_mixed_draw_out(const MixedDraw &d, int n, hipStream_t st)
{
    if (n < 1 || n > kMixedSeqMax || d.vocab < 1 || d.ld < d.vocab || d.logits == nullptr || d.tab == nullptr || d.next == nullptr)
        return hipErrorInvalidValue;
    if (d.sampled && (d.scratch == nullptr || d.row_stride < sample_scratch_floats(d.vocab))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mixed_draw_out, dim3(n), dim3(kSbThreads), 0, st, d);
    return hipGetLastError();
}

}  // namespace l2z
