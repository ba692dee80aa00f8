// prefill_ragged.hip -- what a chunk of the batched prompt pass needs when its rows belong to SEVERAL sequences
// (l2z_prefill_batch; host side: prefill_batch_host.cpp, prefill_host.cpp): the RoPE-and-scatter launch behind the
// q | k | v products, and causal attention in which every row sees its own sequence's cache only.  Everything else of
// the pass treats the rows of a chunk independently and is l2z_prefill's own.
// A row's results depend on its own sequence's rows and caches and on the chunk's table -- never on what the other
// sequences hold (no reduction here crosses a sequence, no block shares state between two).
#include "prefill_common.h"
#include "rope_device.h"

namespace l2z {
namespace {

// One float4 of one row per thread: features [0, dim) are q (rotated in place), [dim, dim + kvd) the key row (rotated, into
// the row's own sequence's key cache at its own position), the last kvd the value row (copied).  The rotation is the
// q | k | v epilogue's (prefill_gemm.hip; main.zig:346-349): pair (v0, v1) -> (v0 c - v1 s, v0 s + v1 c), no fused
// multiply-add.  head_size % 4 == 0: a float4 is two whole pairs of one head.  Vector loads and stores only.
__global__ __launch_bounds__(kPfBlock) void ragged_rope_scatter(float *q, int ldq, const float *k, const float *v,
                                                                const RaggedSeq *seq, const int *row_seq, const int *row_pos,
                                                                int dim, int kvd, int hs, const float2 *rope,
                                                                size_t layer_off, size_t kv_head_stride, size_t page_floats)
{
    const int row = blockIdx.x;
    const int n4 = (dim + 2 * kvd) >> 2;
    const int pos = row_pos[row];
    const RaggedSeq sq = seq[row_seq[row]];
    // where the row's position stands in a (layer, kv head) run of its sequence: row pos of the cache, or (paged) row
    // pos & 63 of the page that holds it
    size_t cache_off = layer_off + (size_t)pos * (size_t)hs;
    if (sq.pages != nullptr) cache_off = (size_t)kv_page_id(sq.pages, pos >> 6) * page_floats + layer_off + (size_t)(pos & 63) * (size_t)hs;
    for (int i = blockIdx.y * kPfBlock + threadIdx.x; i < n4; i += gridDim.y * kPfBlock) {
        int f = 4 * i;
        if (f < dim) {
            float *p = q + (size_t)row * ldq + f;
            const v4f x = *(const v4f *)p;
            *(v4f *)p = rope_rotate4(x, rope_cs4(rope, pos, hs, f));
            continue;
        }
        f -= dim;
        const bool is_k = f < kvd;
        if (!is_k) f -= kvd;
        v4f x = *(const v4f *)((is_k ? k : v) + (size_t)row * kvd + f);
        if (is_k) x = rope_rotate4(x, rope_cs4(rope, pos, hs, f));
        // head-major cache [kv head][seq_len][head_size]
        float *dst = (is_k ? sq.kc : sq.vc) + cache_off + (size_t)(f / hs) * kv_head_stride + (size_t)(f % hs);
        *(v4f *)dst = x;
    }
}

struct RaggedAttnArgs {
    const float *q;
    float *out;
    const RaggedSeq *seq;
    const int *row_seq, *row_pos;
    const int2 *tiles;
    const int *rows;             // the block-per-(head, row) form: != null, block y serves row rows[y] (null: row y)
    size_t layer_off, kv_head;   // floats to this layer in a cache; between kv heads (paged: in a page)
    size_t page_floats;          // paged sequences: floats per page of the pool
    int ldq, ldo, kv_mul, seq_len, head_size;
    __bf16 *x3;                  // != null: out's planes of bf16 terms too (the Wo product's operand)
    int kp;
};

// The general form, every head size the pass takes: block (h, row) is one query and attends to rows 0 .. pos of its own
// sequence's cache.  The arithmetic of the single-sequence block-per-(head, query) kernel (prefill_attention.hip), which
// is the decode kernel's: 256 threads = G groups of TPR lanes.
__global__ __launch_bounds__(kPfBlock) void ragged_attention_rows(const RaggedAttnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int hs = a.head_size, E = hs >> 2;
    int TPR = 1;
    while (TPR < E && TPR < 64) TPR <<= 1;
    const int G = kPfBlock / TPR;
    float *att = lds;                                   // seq_len
    float *part = att + ((a.seq_len + 3) & ~3);         // G*hs
    float *red = part + (size_t)G * hs;                 // 8
    const int h = blockIdx.x, row = a.rows ? a.rows[blockIdx.y] : blockIdx.y;
    const RaggedSeq sq = a.seq[a.row_seq[row]];
    const int T = a.row_pos[row] + 1;
    const int kvh = h / a.kv_mul;
    const float *kbase = sq.kc + a.layer_off + (size_t)kvh * a.kv_head, *vbase = sq.vc + a.layer_off + (size_t)kvh * a.kv_head;
    // key / value row t of this kv head, as floats from kbase / vbase: paged, row t & 63 of the page that holds t
    auto row_off = [&](int t) -> size_t {
        return sq.pages != nullptr ? (size_t)kv_page_id(sq.pages, t >> 6) * a.page_floats + (size_t)(t & 63) * hs : (size_t)t * hs;
    };
    const int g = threadIdx.x / TPR, c0 = threadIdx.x % TPR;
    const bool active = c0 < E;
    const int cc = active ? c0 : 0;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const v4f qv = active ? ((const v4f *)(a.q + (size_t)row * a.ldq + (size_t)h * hs))[cc] : zero;
    const float div = sqrtf((float)hs);
    for (int t = g; t < T; t += G) {
        const v4f kv = ((const v4f *)(kbase + row_off(t)))[cc];
        float p = fmaf(qv.x, kv.x, 0.0f);
        p = fmaf(qv.y, kv.y, p); p = fmaf(qv.z, kv.z, p); p = fmaf(qv.w, kv.w, p);
        for (int o = TPR >> 1; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        if (c0 == 0) att[t] = p / div;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int t = threadIdx.x; t < T; t += blockDim.x) m = fmaxf(m, att[t]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.0f;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const float e = expf(att[t] - m);
        att[t] = e;
        s += e;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = s;
    __syncthreads();
    s = ((red[4] + red[5]) + red[6]) + red[7];
    v4f acc = zero;
    for (int t = g; t < T; t += G) {
        const v4f vv = ((const v4f *)(vbase + row_off(t)))[cc];
        const float w = att[t] / s;  // main.zig:704
        acc.x = fmaf(vv.x, w, acc.x); acc.y = fmaf(vv.y, w, acc.y);
        acc.z = fmaf(vv.z, w, acc.z); acc.w = fmaf(vv.w, w, acc.w);
    }
    if (active) ((v4f *)(part + (size_t)g * hs))[cc] = acc;
    __syncthreads();
    for (int i = threadIdx.x; i < hs; i += blockDim.x) {
        float r = part[i];
        for (int gg = 1; gg < G; gg++) r += part[(size_t)gg * hs + i];
        a.out[(size_t)row * a.ldo + (size_t)h * hs + i] = r;
    }
}

// The flash form, head sizes 64 and 128: block (head, tile) is up to 64 consecutive queries of ONE sequence's segment and
// walks that sequence's cache in tiles of 64 key rows.  The scheme and the arithmetic of the single-sequence flash kernel
// (prefill_attention.hip, where the operand layouts are derived): everything transposed on MFMA 16x16x4 f32, a wave owns 16
// queries and one of the two halves of every key tile, P goes from the S accumulators into the P V product without leaving
// the registers, K / V tiles arrive by direct-to-LDS loads into two buffers.  What differs is where a block finds its
// rows: the segment's first row in the chunk (q, out and the planes), its first position, its row count and its caches
// come from the table.  Masked scores are -inf; key 0 of a sequence is live for every one of its queries.
// PAGED: a key tile is ONE page of the sequence (both are 64 absolute positions): `issue` takes the tile's page id, a
// wave-uniform value read one tile ahead through the scalar path, so no load of the vmcnt-counted ring waits for it;
// the rows, their order in LDS and every sum are the contiguous form's.
template <int NDT, bool PAGED>
__global__ __launch_bounds__(512) void ragged_attention_flash(const RaggedAttnArgs a)
{
    constexpr int KH = 2;
    constexpr int HS = 16 * NDT, E = HS / 4;  // float4 slots per row
    constexpr int NWV = 4 * KH;               // waves: 4 query groups x KH parts of every key tile
    constexpr int JT = 4 / KH;                // 16-row key sub-tiles per wave and tile
    constexpr int LPW = 4 * NDT / NWV;        // wave-wide loads per wave, tile and matrix
    static_assert(NDT == 4 || NDT == 8, "head_size 64 or 128");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int h = blockIdx.x;
    const int2 tile = a.tiles[blockIdx.y];
    const RaggedSeq sq = a.seq[tile.x];
    const int q0 = tile.y, P = sq.rows, pos0 = sq.pos0, seq_len = a.seq_len;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qg = wave & 3, kh = wave >> 2;
    const int qi = lane & 15, g = lane >> 4;
    const int kvh = h / a.kv_mul;  // :369
    const float *kbase = sq.kc + a.layer_off + (size_t)kvh * a.kv_head, *vbase = sq.vc + a.layer_off + (size_t)kvh * a.kv_head;
    const float *q = a.q + (size_t)sq.row0 * a.ldq;
    const int myq = q0 + 16 * qg + qi;              // this lane's query (row of the segment)
    const int qrow = myq < P ? myq : P - 1;         // past the segment: a valid row of it, results dropped
    v4f qreg[NDT];
#pragma unroll
    for (int T = 0; T < NDT; T++) qreg[T] = *(const v4f *)(q + (size_t)qrow * a.ldq + (size_t)h * HS + 16 * T + 4 * g);
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    v4f ot[NDT];
#pragma unroll
    for (int d = 0; d < NDT; d++) ot[d] = zero;
    float m = -INFINITY, lsum = 0.0f;
    const int last_q = (q0 + 63 < P ? q0 + 63 : P - 1);
    const int n_kt = (pos0 + last_q) / 64 + 1;              // key tiles of the block
    const int last_live = pos0 + q0 + 16 * qg + 15;         // last key position live for one of this wave's queries
    const float div = sqrtf((float)HS);
    auto issue = [&](int kt, int buf, int page) {
        const int t0 = kt * 64;
        float *kd = lds + buf * (2 * 64 * HS), *vd = kd + 64 * HS;
        // paged: the tile's rows are rows 0 .. 63 of its page (t0 is a multiple of 64, and seq_len - 1 >= t0 lies in it)
        const float *kt_base = PAGED ? kbase + (size_t)page * a.page_floats - (size_t)t0 * HS : kbase;
        const float *vt_base = PAGED ? vbase + (size_t)page * a.page_floats - (size_t)t0 * HS : vbase;
#pragma unroll
        for (int i = 0; i < LPW; i++) {
            const int f = (wave * LPW + i) * 64 + lane, row = f / E, cp = f % E;
            int t = t0 + row;
            t = t < seq_len ? t : seq_len - 1;  // rows past the context are masked below
            lds_dma16(kt_base + (size_t)t * HS + 4 * (cp ^ (row & 15)), kd + (wave * LPW + i) * 256);
            lds_dma16(vt_base + (size_t)t * HS + 4 * cp, vd + (wave * LPW + i) * 256);
        }
    };
    const int32_t *pages = PAGED ? sq.pages : nullptr;
    int page_next = 0;   // the page of the tile `issue` takes next
    if (PAGED) page_next = kv_page_id(pages, 0);
    issue(0, 0, page_next);
    if (PAGED && n_kt > 1) page_next = kv_page_id(pages, 1);
    for (int kt = 0; kt < n_kt; kt++) {
        const int t0 = kt * 64;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of tile kt has landed
        __syncthreads();  // everyone's has; and every wave is done with tile kt - 1: its buffer is free
        if (kt + 1 < n_kt) {
            issue(kt + 1, (kt + 1) & 1, page_next);
            if (PAGED && kt + 2 < n_kt) page_next = kv_page_id(pages, kt + 2);
        }
        const float *ks = lds + (kt & 1) * (2 * 64 * HS), *vs = ks + 64 * HS;
        const int r0 = (64 / KH) * kh;                 // this wave's rows of the tile
        if (t0 + r0 > last_live) continue;             // nothing live for this wave (wave-uniform)
        v4f st[JT];
#pragma unroll
        for (int jt = 0; jt < JT; jt++) st[jt] = zero;
#pragma unroll
        for (int T = 0; T < NDT; T++)
#pragma unroll
            for (int jt = 0; jt < JT; jt++) {
                const int row = r0 + 16 * jt + qi;
                const v4f kq = ((const v4f *)(ks + row * HS))[(4 * T + g) ^ (row & 15)];
#pragma unroll
                for (int c = 0; c < 4; c++)
                    st[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kq[c], qreg[T][c], st[jt], 0, 0, 0);
            }
        float mx = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < JT; jt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool live = t0 + r0 + 16 * jt + 4 * g + r <= pos0 + myq;  // t <= pos of the query
                st[jt][r] = live ? st[jt][r] / div : -INFINITY;                 // :372
                mx = fmaxf(mx, st[jt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float mref = m_new == -INFINITY ? 0.0f : m_new;   // (no live key seen yet: every weight e^(-inf) = 0)
        float sum = 0.0f;
#pragma unroll
        for (int jt = 0; jt < JT; jt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                st[jt][r] = expf(st[jt][r] - mref);
                sum += st[jt][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float alpha = expf(m - mref);  // first live tile: e^(-inf) = 0
        lsum = lsum * alpha + sum;
        m = m_new;
#pragma unroll
        for (int d = 0; d < NDT; d++) ot[d] *= alpha;
#pragma unroll
        for (int DT = 0; DT < NDT / 4; DT++)
#pragma unroll
            for (int jt = 0; jt < JT; jt++)
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const v4f vq = *(const v4f *)(vs + (r0 + 16 * jt + 4 * g + s4) * HS + 4 * (16 * DT + qi));
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        ot[4 * DT + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[c], st[jt][s4], ot[4 * DT + c], 0, 0, 0);
                }
    }
    {
        // the two key parts of a query group: merge (m, l, O) of the upper part into the lower one
        __syncthreads();  // K / V buffers are free
        float *mg = lds + (size_t)(qg * 64 + lane) * (4 * NDT + 2);
        if (kh == 1) {
#pragma unroll
            for (int d = 0; d < NDT; d++)
#pragma unroll
                for (int r = 0; r < 4; r++) mg[4 * d + r] = ot[d][r];
            mg[4 * NDT] = m;
            mg[4 * NDT + 1] = lsum;
        }
        __syncthreads();
        if (kh == 1) return;
        const float m1 = mg[4 * NDT], l1 = mg[4 * NDT + 1];
        const float mm = fmaxf(m, m1);  // finite: the lower part holds key 0
        const float a0 = expf(m - mm), a1 = expf(m1 - mm);
        lsum = lsum * a0 + l1 * a1;
#pragma unroll
        for (int d = 0; d < NDT; d++)
#pragma unroll
            for (int r = 0; r < 4; r++) ot[d][r] = ot[d][r] * a0 + mg[4 * d + r] * a1;
    }
    // ot[4 DT + c][r] = O^T[d = 64 DT + 16 g + 4 r + c][query myq]: 16 consecutive d per (lane, DT)
    if (myq < P) {
        const int crow = sq.row0 + myq;   // the query's row in the chunk
        float *o = a.out + (size_t)crow * a.ldo + (size_t)h * HS;
#pragma unroll
        for (int DT = 0; DT < NDT / 4; DT++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                v4f v;
#pragma unroll
                for (int c = 0; c < 4; c++) v[c] = ot[4 * DT + c][r] / lsum;  // :704
                *(v4f *)(o + 64 * DT + 16 * g + 4 * r) = v;
                if (a.x3) planes_store4(a.x3, a.kp, crow, h * HS + 64 * DT + 16 * g + 4 * r, v);
            }
    }
}

}  // namespace

hipError_t launch_ragged_rope_scatter(float *q, int ldq, const RaggedChunk &rg, int P, int dim, int kv_dim, int head_size,
                                      const float2 *rope, size_t layer_off, size_t kv_head_stride, hipStream_t st)
{
    if (rg.page_floats & 3) return hipErrorInvalidValue;
    if (P <= 0 || (head_size & 3) || (dim % head_size) || (kv_dim % head_size) || (ldq & 3) ||
        (((uintptr_t)q | (uintptr_t)rg.k | (uintptr_t)rg.v | (uintptr_t)rope) & 15) || (layer_off & 3) || (kv_head_stride & 3))
        return hipErrorInvalidValue;
    const int n4 = (dim + 2 * kv_dim) >> 2;
    const dim3 grid(P, (n4 + 4 * kPfBlock - 1) / (4 * kPfBlock));   // up to four float4 per thread
    hipLaunchKernelGGL(ragged_rope_scatter, grid, dim3(kPfBlock), 0, st, q, ldq, (const float *)rg.k, (const float *)rg.v, rg.seq,
                       rg.row_seq, rg.row_pos, dim, kv_dim, head_size, rope, layer_off, kv_head_stride, rg.page_floats);
    return hipGetLastError();
}

hipError_t launch_ragged_attention(const RaggedLayer &L, const RaggedChunk &rg, bool *planes_written)
{
    const int P = L.P, head_size = L.head_size;
    if (planes_written) *planes_written = false;
    if (P <= 0 || (head_size & 3) || head_size > 256 || rg.n_seq < 1 || rg.n_seq > rg.seq_max ||
        (rg.att_rows != nullptr && (rg.n_att_rows < 1 || rg.n_att_rows > P)))
        return hipErrorInvalidValue;
    RaggedAttnArgs a = {};
    a.q = L.q; a.out = L.out; a.seq = rg.seq; a.row_seq = rg.row_seq; a.row_pos = rg.row_pos; a.tiles = rg.tiles;
    a.layer_off = L.layer_off; a.kv_head = L.kv_head_stride; a.ldq = L.ldq; a.ldo = L.ldo; a.kv_mul = L.kv_mul; a.seq_len = L.seq_len;
    a.head_size = head_size; a.page_floats = rg.page_floats; a.rows = rg.att_rows;
    // (the caches come from hipMalloc and a layer / a kv head is a multiple of head_size floats: 16-byte aligned rows)
    if ((head_size == 64 || head_size == 128) && (L.ldq % 4) == 0 && (L.ldo % 4) == 0 && rg.n_tiles > 0 &&
        (((uintptr_t)L.q | (uintptr_t)L.out) & 15) == 0) {
        const size_t lds_f = (size_t)2 * 2 * 64 * head_size * sizeof(float);  // two buffers of a K and a V tile
        const bool paged = rg.page_floats != 0;
        const void *fn = head_size == 128
                             ? (paged ? (const void *)ragged_attention_flash<8, true> : (const void *)ragged_attention_flash<8, false>)
                             : (paged ? (const void *)ragged_attention_flash<4, true> : (const void *)ragged_attention_flash<4, false>);
        if (lds_f > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f);
            if (e != hipSuccess) return e;
        }
        if (L.x3 != nullptr && (L.kp & 3) == 0) { a.x3 = (__bf16 *)L.x3; a.kp = L.kp; }
        if (planes_written) *planes_written = a.x3 != nullptr;
        void *params[] = {(void *)&a};
        return hipLaunchKernel(fn, dim3(L.n_heads, rg.n_tiles), dim3(512), params, lds_f, L.st);
    }
    int E = head_size >> 2, TPR = 1;
    while (TPR < E && TPR < 64) TPR <<= 1;
    const int G = kPfBlock / TPR;
    const size_t lds = (size_t)(((L.seq_len + 3) & ~3) + G * head_size + 8) * sizeof(float);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ragged_attention_rows),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ragged_attention_rows, dim3(L.n_heads, rg.att_rows != nullptr ? rg.n_att_rows : P), dim3(kPfBlock), lds, L.st, a);
    return hipGetLastError();
}

}  // namespace l2z
