// matvec_device.h -- device helpers of the mat-vec kernels (matvec.hip): the argument block copied into locals,
// the pair -> weight rows map, and the fused epilogues (RoPE + KV write, residual, SwiGLU, store) with what they
// prefetch; and, host side, how the launchers size a grid.  Anonymous namespace, like kernel_common.h.
#pragma once
#include "kernel_common.h"

namespace l2z {
namespace {

// Kernel arguments copied into plain locals once (keeps them out of scratch).
struct MvLocals {
    const float *w0, *w1, *w2;
    float *out0, *out1, *out2;
    const float *resid;
    const float2 *rope;
    int rows0, r01, total_rows, n_pairs, n, head_size, rope_segs, pos;
    size_t ps1, ps2;
    size_t kv_head_stride;  // != 0: out1 / out2 are head-major caches (MatvecArgs::kv_head_stride)
    const P2pArgs *push;  // sharded: LL words of the outputs go straight to the peers
    int push_e;
    size_t push_base;     // index of out0[0] in the gathered vector
    const uint32_t *pk, *pk1, *pk2;  // packed slots of w0 / w1 / w2 (MatvecArgs::pk...; packed row kernel only)
    int pk_e, pk_e1, pk_e2;
    const uint32_t *pk_rec, *pk_rec1, *pk_rec2;  // the 28-bit form's patch records (MatvecArgs::pk_rec...)
};

template <int EPI>
__device__ __forceinline__ MvLocals mv_locals(const MatvecArgs &a)
{
    MvLocals m;
    m.w0 = a.w0; m.w1 = a.w1; m.w2 = a.w2;
    m.out0 = a.out0; m.out1 = a.out1; m.out2 = a.out2;
    m.resid = a.resid; m.rope = a.rope;
    m.rows0 = a.rows0; m.r01 = a.rows0 + a.rows1; m.total_rows = a.rows0 + a.rows1 + a.rows2;
    m.n_pairs = (EPI == EPI_SWIGLU) ? a.rows0 : (m.total_rows + 1) >> 1;
    m.n = a.n; m.head_size = a.head_size; m.rope_segs = a.rope_segs;
    m.pos = (EPI == EPI_ROPE) ? *a.pos_ptr : 0;
    m.ps1 = (size_t)m.pos * (size_t)a.pos_stride1;
    m.ps2 = (size_t)m.pos * (size_t)a.pos_stride2;
    m.kv_head_stride = (EPI == EPI_ROPE) ? a.kv_head_stride : 0;
    m.push = a.push;
    m.push_e = m.push ? a.push_ctl[kCtlEpoch] + a.push_gi : 0;
    m.push_base = m.push ? (size_t)m.push->rank * m.push->count : 0;
    m.pk = a.pk; m.pk1 = a.pk1; m.pk2 = a.pk2;
    m.pk_e = a.pk_e; m.pk_e1 = a.pk_e1; m.pk_e2 = a.pk_e2;
    m.pk_rec = a.pk_rec; m.pk_rec1 = a.pk_rec1; m.pk_rec2 = a.pk_rec2;
    return m;
}

// Global row g of the concatenated row space -> the segment (0 / 1 / 2: w0 / w1 / w2, out0 / out1 / out2) it lies in
// and its row within that segment
struct SegRow {
    bool past0, past1;  // at or past the end of segment 0 / of segment 1: the segment as the two compares that find it
    int row;
    __device__ __forceinline__ int seg() const { return past1 ? 2 : (past0 ? 1 : 0); }
    // one of three per-segment values, as two selects
    template <typename T>
    __device__ __forceinline__ T pick(T v0, T v1, T v2) const
    {
        const T v = past0 ? v1 : v0;
        return past1 ? v2 : v;
    }
};

__device__ __forceinline__ SegRow seg_row(const MvLocals &m, int g)
{
    SegRow r;
    r.past0 = g >= m.rows0;
    r.past1 = g >= m.r01;
    r.row = g - (r.past1 ? m.r01 : (r.past0 ? m.rows0 : 0));
    return r;
}

// the two weight rows of pair p (clamped to the last pair for idle lane groups)
template <int EPI>
__device__ __forceinline__ void pair_rows(const MvLocals &m, int p, const float *&pa, const float *&pb)
{
    if (p >= m.n_pairs) p = m.n_pairs - 1;
    if (EPI == EPI_SWIGLU) {  // w0: W1 | W3 row-interleaved (MatvecArgs): the pair is one contiguous run like any other
        pa = m.w0 + (size_t)(2 * p) * (size_t)m.n;
        pb = pa + m.n;
    } else {
        const int ga = 2 * p;
        const int gb = (ga + 1 < m.total_rows) ? ga + 1 : ga;
        const SegRow ra = seg_row(m, ga), rb = seg_row(m, gb);
        pa = ra.pick(m.w0, m.w1, m.w2) + (size_t)ra.row * (size_t)m.n;
        pb = rb.pick(m.w0, m.w1, m.w2) + (size_t)rb.row * (size_t)m.n;
    }
}

// packed form of pair_rows: the 29-bit chunks of pair p (pair_dw dwords, packed_w.h) and its slot's base exponent.  A
// pair is rows 2q, 2q + 1 of ONE slot (packed slots have an even number of rows); only q | k | v has three slots
template <int EPI>
__device__ __forceinline__ const uint32_t *pair_packed(const MvLocals &m, int p, size_t pair_dw, int &e_base)
{
    if (p >= m.n_pairs) p = m.n_pairs - 1;
    if (EPI == EPI_ROPE) {
        const SegRow r = seg_row(m, 2 * p);
        e_base = r.pick(m.pk_e, m.pk_e1, m.pk_e2);
        return r.pick(m.pk, m.pk1, m.pk2) + (size_t)(r.row >> 1) * pair_dw;
    }
    e_base = m.pk_e;
    return m.pk + (size_t)p * pair_dw;
}

// ... and of the 28-bit form (packed_w.h pk28): the pair's stream, of pair_dw dwords, and its patch record of rec_dw
template <int EPI>
__device__ __forceinline__ const uint32_t *pair_packed28(const MvLocals &m, int p, size_t pair_dw, size_t rec_dw, int &e_base,
                                                         const uint32_t *&rec)
{
    if (p >= m.n_pairs) p = m.n_pairs - 1;
    if (EPI == EPI_ROPE) {
        const SegRow r = seg_row(m, 2 * p);
        const size_t q = (size_t)(r.row >> 1);
        e_base = r.pick(m.pk_e, m.pk_e1, m.pk_e2);
        rec = r.pick(m.pk_rec, m.pk_rec1, m.pk_rec2) + q * rec_dw;
        return r.pick(m.pk, m.pk1, m.pk2) + q * pair_dw;
    }
    e_base = m.pk_e;
    rec = m.pk_rec + (size_t)p * rec_dw;
    return m.pk + (size_t)p * pair_dw;
}

// What the epilogue of pair p reads from memory (residual values, RoPE cos/sin).  Loaded by
// the writer lane when the pair's weight loads are issued, so the epilogue itself never
// waits on memory (a dependent L2 round trip per unit otherwise: ~1 us, serialised).
struct EpiIn {
    float ra, rb;
    float2 cs;
};

template <int EPI>
__device__ __forceinline__ EpiIn epi_prefetch(const MvLocals &m, int p, bool writer)
{
    EpiIn e;
    e.ra = 0.0f; e.rb = 0.0f; e.cs = make_float2(1.0f, 0.0f);
    if (!writer || p >= m.n_pairs) return e;
    if (EPI == EPI_RESID) {  // single segment: rows 2p, 2p+1
        const int ga = 2 * p, gb = ga + 1;
        e.ra = m.resid[ga];
        if (gb < m.total_rows) e.rb = m.resid[gb];
    } else if (EPI == EPI_ROPE) {
        const SegRow ra = seg_row(m, 2 * p);
        if (ra.seg() < m.rope_segs) {
            const int hs = m.head_size;
            e.cs = m.rope[(size_t)m.pos * (size_t)(hs >> 1) + (size_t)((ra.row % hs) >> 1)];
        }
    }
    return e;
}

template <int EPI>
__device__ __forceinline__ void pair_epilogue(const MvLocals &m, int p, float sa, float sb, bool writer, const EpiIn &in)
{
    const bool valid_a = p < m.n_pairs;
    if (EPI == EPI_SWIGLU) {
        float v = sa;
        v = v * (1.0f / (1.0f + expf(-v)));  // :412
        v = v * sb;                          // :416
        if (writer && valid_a) {
            m.out0[p] = v;
            if (m.push) p2p_ll_push(m.push, m.push_e, m.push_base + (size_t)p, v);
        }
        return;
    }
    const int ga = 2 * p, gb = ga + 1;
    const bool valid_b = valid_a && gb < m.total_rows;
    const SegRow ra = seg_row(m, ga), rb = seg_row(m, gb);
    const int row_a = ra.row, row_b = rb.row;
    float *oa = ra.pick(m.out0, m.out1 + m.ps1, m.out2 + m.ps2);
    float *ob = rb.pick(m.out0, m.out1 + m.ps1, m.out2 + m.ps2);
    if (EPI == EPI_ROPE) {
        // rows (row_a, row_a+1) of one segment: the pair (i, i+1) of :346-349
        float o0 = sa, o1 = sb;
        if (ra.seg() < m.rope_segs) {
            const float2 cs = in.cs;     // rope[pos][(row_a % head_size)/2], prefetched
            o0 = sa * cs.x - sb * cs.y;  // :348
            o1 = sa * cs.y + sb * cs.x;  // :349
        }
        if (writer && valid_a) {  // q, or the pos row of the K / V cache (:354-358)
            size_t ia = (size_t)row_a, ib = (size_t)row_b;
            if (m.kv_head_stride) {  // head-major cache: [kv head][pos][i]; ps1 / ps2 = pos * head_size
                const int hs = m.head_size;
                if (ra.past0) ia = (size_t)(row_a / hs) * m.kv_head_stride + (size_t)(row_a % hs);
                if (rb.past0) ib = (size_t)(row_b / hs) * m.kv_head_stride + (size_t)(row_b % hs);
            }
            oa[ia] = o0;
            if (valid_b) ob[ib] = o1;
        }
    } else if (EPI == EPI_RESID) {
        if (writer && valid_a) {
            const float va = in.ra + sa, vb = in.rb + sb;  // :711 a[i] += b[i]  (resid[row] prefetched)
            oa[row_a] = va;
            if (valid_b) ob[row_b] = vb;
            if (m.push) {  // single segment on this path: row == index in the slice
                p2p_ll_push(m.push, m.push_e, m.push_base + (size_t)row_a, va);
                if (valid_b) p2p_ll_push(m.push, m.push_e, m.push_base + (size_t)row_b, vb);
            }
        }
    } else {
        if (writer && valid_a) {
            oa[row_a] = sa;
            if (valid_b) ob[row_b] = sb;
            if (m.push) {
                p2p_ll_push(m.push, m.push_e, m.push_base + (size_t)row_a, sa);
                if (valid_b) p2p_ll_push(m.push, m.push_e, m.push_base + (size_t)row_b, sb);
            }
        }
    }
}

// ---- host side: the grid of a mat-vec launch (launch_matvec, launch_q8_matvec) ----
// Blocks resident at once -- a launch has no more, so every block pays its prologue once --: what the occupancy query
// gives the kernel with its LDS, at most blocks_per_cu a CU, at most grid_cap in all (0: no such cap)
inline int mv_resident_blocks(const void *fn, size_t lds, int blocks_per_cu, int n_cus, int grid_cap)
{
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kBlock, lds) != hipSuccess || occ < 1) occ = 1;
    if (occ > blocks_per_cu) occ = blocks_per_cu;
    const int resident = occ * n_cus;
    return grid_cap > 0 && resident > grid_cap ? grid_cap : resident;
}
// the row kernel: a unit per block at a time, every block the same count +-1
inline int mv_grid_block_units(int n_units, int resident)
{
    if (n_units <= resident) return n_units;
    const int per_block = (n_units + resident - 1) / resident;
    return (n_units + per_block - 1) / per_block;
}
// kernels whose waves own the units (matvec_kernel, matvec_scalar_kernel, q8_matvec_kernel): dealt round-robin, every
// wave the same count +-1
inline int mv_grid_wave_units(int n_units, int resident)
{
    const int blocks_needed = (n_units + kWaves - 1) / kWaves;
    if (blocks_needed <= resident) return blocks_needed;
    const int per_wave = (n_units + resident * kWaves - 1) / (resident * kWaves);
    return (n_units + per_wave * kWaves - 1) / (per_wave * kWaves);
}

}  // namespace
}  // namespace l2z
