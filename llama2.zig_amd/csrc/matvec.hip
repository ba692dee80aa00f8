// matvec.hip (with attention.hip, misc_kernels.hip, kernel_common.h) -- hand-written gfx950
// (CDNA4, wave64) kernels for the llama2.zig forward pass.  Every kernel cites the reference lines (src/main.zig) whose
// arithmetic it performs.  Compiled with -ffp-contract=off: every fused
// multiply-add below is an explicit fmaf(), everything else rounds once per
// operation exactly like the reference's scalar code.
//
// Design (DESIGN.md has the numbers):
//  * mat-vec is pure HBM streaming (0.5 flop/byte): one wave owns two weight
//    rows at a time, each lane issues 16-byte non-temporal loads (1 KiB per
//    wave-instruction, 8 in flight per lane), x is staged once per block in
//    LDS, dot products finish with a wave-wide xor-shuffle reduction.  One
//    fixed summation order per output row => results do not depend on grid
//    size or on how rows are sharded over GPUs.
//  * what the reference does immediately before / after each matmul is fused
//    into that launch: rmsnorm (prologue), RoPE + KV-cache write, residual
//    add, SiLU*mul (epilogues).  5 launches per layer.
//  * token and position live in device memory so one captured hipGraph per
//    step can be replayed without host involvement.
// matvec.hip: the fused mat-vec kernels (narrow rows, wide rows, generic scalar) and their launcher.
#include <type_traits>

#include "argmax_rule.h"
#include "matvec_device.h"
#include "packed_w.h"

namespace l2z {
namespace {

// Two dot products against the staged x, generic scalar form (any n / alignment).
__device__ __forceinline__ void dot2_scalar(const float *__restrict__ pa,
                                            const float *__restrict__ pb, const float *xs, int n,
                                            float &ra, float &rb)
{
    const int lane = threadIdx.x & 63;
    float sa = 0.0f, sb = 0.0f;
    for (int j = lane; j < n; j += kWave) {
        const float xv = xs[j];
        sa = fmaf(pa[j], xv, sa);
        sb = fmaf(pb[j], xv, sb);
    }
    ra = wave_sum(sa);
    rb = wave_sum(sb);
}

// ---------------------------------------------------------------------------
// The fused mat-vec.  main.zig:530-605 matmul_fused with its neighbours:
//   PRO_RMS    rmsnorm before it                   :305 / :398 / :426
//   EPI_ROPE   RoPE on q,k + KV-cache row write    :336-358
//   EPI_RESID  accum into the residual stream      :395 / :422
//   EPI_SWIGLU silu(w1.x) * (w3.x)                 :411-416
//
// Work decomposition.  A "pair" is two weight rows that share x reads (rows
// 2p,2p+1 of the concatenated row space -- exactly the RoPE pair (i,i+1) -- or
// row p of w1 and of w3 for SwiGLU).  LPR lanes cooperate on one pair, so a
// wave works on 64/LPR pairs at once:
//   LPR = 64 : large n (7B shapes): one pair per wave, 1 KiB per load instruction
//   LPR < 64 : small n (stories15M/110M): several pairs per wave so that all 64
//              lanes load 16 B and a whole row is in flight at once
// Lane cl of a group takes float4 columns cl, cl+LPR, ... in increasing order
// into 4 component accumulators, then (x+y)+(z+w), then an xor-shuffle over the
// group.  LPR is a function of n only, so a row's summation order never
// depends on the grid, the row count or how rows are sharded over GPUs.
//
// Latency.  Each wave issues the loads of its first weight batch BEFORE the
// block stages x (x's own loads are issued first and return first), so HBM
// latency overlaps the rmsnorm prologue instead of following it.
//
// All kernel arguments are read into scalars and selected with arithmetic:
// indexing the by-value argument block dynamically pushes it into scratch.
// ---------------------------------------------------------------------------
template <int LPR>
struct MvGeom {
    static constexpr int RW = kWave / LPR;          // pairs per wave
    static constexpr int U = (LPR == 64) ? 4 : 6;   // float4 per row per lane per batch
};

// Issue one batch: U float4 of row a and of row b at columns c0 + k*LPR.  Columns past
// the row end are clamped to its last float4: the matching x entries in LDS are the
// zero padding, so they add exactly 0 (weights are finite) -- no predicated loads.
template <int LPR>
__device__ __forceinline__ void mv_load(const float *pa, const float *pb, int c0, int n4,
                                        v4f (&wa)[MvGeom<LPR>::U], v4f (&wb)[MvGeom<LPR>::U])
{
    constexpr int U = MvGeom<LPR>::U;
    const v4f *a4 = (const v4f *)pa, *b4 = (const v4f *)pb;
    // Per lane: n4 need not be a multiple of the lane count -- the last step of a row like hidden_dim 1376
    // (n4 = 344 = 5 * 64 + 24) is a partial one, the vector form of the reference's scalar tail
    // (main.zig:589-594).
#pragma unroll
    for (int k = 0; k < U; k++) {
        int c = c0 + LPR * k;
        c = c < n4 ? c : n4 - 1;
        wa[k] = ldg_nt(a4 + c);
        wb[k] = ldg_nt(b4 + c);
    }
}

template <int LPR>
__device__ __forceinline__ void mv_consume(const v4f *xs4, int c0, const v4f (&wa)[MvGeom<LPR>::U],
                                           const v4f (&wb)[MvGeom<LPR>::U], v4f &acc_a, v4f &acc_b)
{
    constexpr int U = MvGeom<LPR>::U;
#pragma unroll
    for (int k = 0; k < U; k++) {
        const v4f xv = xs4[c0 + LPR * k];  // zero padded to whole batches
        acc_a = fma4(wa[k], xv, acc_a);
        acc_b = fma4(wb[k], xv, acc_b);
    }
}

// One step of the flat (unit, batch) loop of both vector kernels: after batch b of unit u comes batch b + 1 of the same
// unit, or batch 0 of the unit ustride further on; `more` = there is such a batch.
struct MvStep {
    bool unit_done, more;
    int u_next, b_next;
};

__device__ __forceinline__ MvStep mv_step(int u, int b, int n_batches, int ustride, int n_units)
{
    MvStep s;
    s.unit_done = (b + 1 == n_batches);
    s.u_next = s.unit_done ? u + ustride : u;
    s.b_next = s.unit_done ? 0 : b + 1;
    s.more = s.u_next < n_units;
    return s;
}

template <int PRO, int EPI, int LPR, int XC, bool LL>
__global__ __launch_bounds__(kBlock) void matvec_kernel(const MatvecArgs a)
{
    using G = MvGeom<LPR>;
    constexpr int U = G::U, RW = G::RW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MvLocals m = mv_locals<EPI>(a);
    const int n4 = m.n >> 2;
    const int n_batches = (n4 + LPR * U - 1) / (LPR * U);
    const int n4_pad = n_batches * (LPR * U);
    float *xs = lds;
    float *scratch = lds + 4 * n4_pad;
    const v4f *xs4 = (const v4f *)xs;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / LPR, cl = lane % LPR;
    const int n_units = (m.n_pairs + RW - 1) / RW;
    const int ustride = gridDim.x * kWaves;

    // 1. issue x loads (they return first), 2. issue the first weight batch, 3. stage x
    XStage<PRO, XC, LL> xst;
    xst.issue(a.x, a.xin, a.rms_w, n4);
    int u = blockIdx.x * kWaves + wave;
    const bool has_unit = u < n_units;
    const float *pa, *pb;
    pair_rows<EPI>(m, (has_unit ? u : 0) * RW + grp, pa, pb);
    v4f wa[U], wb[U];
    EpiIn ein = epi_prefetch<EPI>(m, (has_unit ? u : 0) * RW + grp, cl == 0 && has_unit);
    EpiIn ein_next = ein;
    mv_load<LPR>(pa, pb, cl, n4, wa, wb);
    xst.finish(a.x, a.rms_w, m.n, n4_pad, xs, scratch);
    if (EPI != EPI_ARGMAX && !has_unit) return;

    // flat loop over (unit, batch): consume the batch in registers, then immediately
    // issue the next one -- the next unit's first batch included -- before reducing
    v4f acc_a = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    ArgmaxCand best;  // EPI_ARGMAX: running (max, first index) of this lane's rows
    int b = 0;
    while (has_unit) {
        mv_consume<LPR>(xs4, cl + b * (LPR * U), wa, wb, acc_a, acc_b);
        const MvStep s = mv_step(u, b, n_batches, ustride, n_units);
        if (s.more) {
            if (s.unit_done) {
                pair_rows<EPI>(m, s.u_next * RW + grp, pa, pb);
                ein_next = epi_prefetch<EPI>(m, s.u_next * RW + grp, cl == 0);
            }
            mv_load<LPR>(pa, pb, cl + s.b_next * (LPR * U), n4, wa, wb);
        }
        if (s.unit_done) {
            const float sa = lanes_sum(hsum4(acc_a), LPR);
            const float sb = lanes_sum(hsum4(acc_b), LPR);
            pair_epilogue<EPI>(m, u * RW + grp, sa, sb, cl == 0, ein);
            ein = ein_next;
            if (EPI == EPI_ARGMAX) {  // single segment: pair p = rows 2p, 2p+1, taken in increasing order
                const int ra_ = 2 * (u * RW + grp), rb_ = ra_ + 1;
                if (ra_ < m.total_rows) argmax_take(best, sa, ra_ + a.row_offset);
                if (rb_ < m.total_rows) argmax_take(best, sb, rb_ + a.row_offset);
            }
            acc_a = v4f{0.f, 0.f, 0.f, 0.f};
            acc_b = v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (!s.more) break;
        u = s.u_next;
        b = s.b_next;
    }
    if (EPI == EPI_ARGMAX) {
        // block candidate: larger value wins, equal values -> lower index, the NaN at row 0 above all (argmax_rule.h)
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
            a.part_val[blockIdx.x] = c.v;
            a.part_idx[blockIdx.x] = c.i;
        }
    }
}

// Packed weights (PK, packed_w.h): the raw dwords of one lane's chunk of a batch.  Plane q of 16 bytes per lane lands
// in q4[q], single-dword plane r in q1[r]: fixed registers whatever the step count S, so a chunk of a runtime S is
// loaded with wave-uniform predicates and no register is indexed at run time
struct PkRaw {
    v4u q4[7];
    uint32_t q1[3];
};

__device__ __forceinline__ void pk_load_raw(const uint32_t *src, int lane, int s, PkRaw &r)
{
    const int q = pk::lane_dw(s) / 4, rem = pk::lane_dw(s) % 4;
#pragma unroll
    for (int i = 0; i < 7; i++)
        if (i < q) r.q4[i] = __builtin_nontemporal_load((const v4u *)(src + i * 256 + lane * 4));
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (i < rem) r.q1[i] = __builtin_nontemporal_load(src + q * 256 + i * 64 + lane);
}

// ... and its values, exactly the f32 bits, into the fp32 kernel's registers; steps past the row end are zero there too
template <int S>
__device__ __forceinline__ void pk_decode_lane(const PkRaw &r, int e31, v4f (&wa)[4], v4f (&wb)[4])
{
    constexpr int N = pk::lane_dw(S), Q = N / 4;
    uint32_t d[N > 0 ? N : 1], t[8 * S > 0 ? 8 * S : 1];
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (i < 4 * Q) {
            const v4u v = r.q4[i / 4];
            d[i] = (i % 4 == 0) ? v.x : (i % 4 == 1) ? v.y : (i % 4 == 2) ? v.z : v.w;
        } else {
            d[i] = r.q1[i - 4 * Q];
        }
    }
    pk::decode_lane_t<S>(d, t);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < S) {
            wa[k] = v4f{__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k]), e31), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 1]), e31),
                        __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 2]), e31), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 3]), e31)};
            wb[k] = v4f{__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 4]), e31), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 5]), e31),
                        __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 6]), e31), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 7]), e31)};
        } else {
            wa[k] = v4f{0.f, 0.f, 0.f, 0.f};
            wb[k] = v4f{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// Where matvec_row_kernel's (unit, batch) loop gets a batch's wa[] / wb[] from.  A source offers
//   point(m, u)   aim at unit u's pair,
//   issue<P>(b)   request batch b of that pair into register set P,
//   deliver<P>()  wa[] / wb[] hold the batch of set P for the FMAs,
// and kSets says when the loop requests the next batch: 1 = after the current batch's FMAs, into the same registers
// (fp32); 2 = before the current batch is decoded, into the other of two FIXED sets of raw words that the loop, unrolled
// twice, takes in turn (packed): no set is ever copied into the other, so a request never waits for an earlier batch.
constexpr int kRowU = 4;  // float4 per row per thread per batch

template <int EPI, int XC>
struct RowF32 {
    static constexpr int kSets = 1;
    v4f wa[kRowU], wb[kRowU];
    const float *pa, *pb;
    int n4;

    __device__ __forceinline__ void init(const MvLocals &, int n4_, int) { n4 = n4_; }
    __device__ __forceinline__ void point(const MvLocals &m, int u) { pair_rows<EPI>(m, u, pa, pb); }
    template <int P>
    __device__ __forceinline__ void issue(int b)
    {
        // columns cb + tid + 256k; validity is wave-uniform (n4 % 64 == 0)
        const int tid = threadIdx.x, cb = b * (kBlock * kRowU);
        const v4f *a4 = (const v4f *)pa + cb + tid, *b4 = (const v4f *)pb + cb + tid;
        const int wbase = cb + (tid & ~63);
#pragma unroll
        for (int k = 0; k < kRowU; k++) {
            const bool in_row = wbase + kBlock * k < n4;  // wave-uniform
            if (XC == 12 && !in_row) {
                // rows that do not fill their last batch (n = 11008: 704 of 1024 float4): the out-of-row steps
                // load NOTHING (their x is the zero padding) -- the re-reads of the row start were 11.6 % of
                // W2's load instructions and, the nt lines long evicted, 2.7 % extra HBM traffic (PMC 1.027x)
                wa[k] = v4f{0.f, 0.f, 0.f, 0.f};
                wb[k] = v4f{0.f, 0.f, 0.f, 0.f};
                continue;
            }
            const int off = in_row ? kBlock * k : -(cb + (tid & ~63));
            wa[k] = ldg_nt(a4 + off);  // out-of-row steps re-read the row start; their x is 0
            wb[k] = ldg_nt(b4 + off);
        }
    }
    template <int P>
    __device__ __forceinline__ void deliver() {}
};

template <int EPI, int XC>
struct RowPacked {
    static constexpr int kSets = 2;
    v4f wa[kRowU], wb[kRowU];
    // per set: the raw words of a batch, its in-row steps and its slot's exponent offset (both wave-uniform)
    PkRaw raw[kSets];
    int s_in[kSets], e31[kSets];
    const uint32_t *pp;
    size_t pdw, last_off;
    int e_pt, s_last, wave_u, n_batches;

    __device__ __forceinline__ void init(const MvLocals &, int n4, int n_batches_)
    {
        n_batches = n_batches_;
        wave_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        pdw = pk::pair_dw(n4);
        last_off = pk::chunk_off(n4, n_batches - 1, wave_u);
        s_last = pk::steps(n4, n_batches - 1, wave_u);
    }
    __device__ __forceinline__ void point(const MvLocals &m, int u)
    {
        int e;
        pp = pair_packed<EPI>(m, u, pdw, e);
        e_pt = e - 31;
    }
    template <int P>
    __device__ __forceinline__ void issue(int b)
    {
        const bool last = b + 1 == n_batches;
        const uint32_t *src = pp + (last ? last_off : (size_t)b * (4 * 64 * pk::kMaxLaneDw) + (size_t)wave_u * (64 * pk::kMaxLaneDw));
        s_in[P] = (XC == 4 || !last) ? 4 : s_last;  // n = 4096: one full batch
        e31[P] = e_pt;
        pk_load_raw(src, threadIdx.x & 63, XC == 4 ? 4 : s_in[P], raw[P]);
    }
    template <int P>
    __device__ __forceinline__ void deliver()
    {
        if constexpr (XC == 4) {
            pk_decode_lane<4>(raw[P], e31[P], wa, wb);
        } else {
            switch (s_in[P]) {  // wave-uniform
                case 4: pk_decode_lane<4>(raw[P], e31[P], wa, wb); break;
                case 3: pk_decode_lane<3>(raw[P], e31[P], wa, wb); break;
                case 2: pk_decode_lane<2>(raw[P], e31[P], wa, wb); break;
                case 1: pk_decode_lane<1>(raw[P], e31[P], wa, wb); break;
                default: pk_decode_lane<0>(raw[P], e31[P], wa, wb); break;
            }
        }
    }
};

// The 28-bit form (packed_w.h pk28) of a pair whose rows are exactly one batch (XC == 4): the same two fixed sets, seven
// 16-byte loads a lane and batch, and the pair's patch record -- 16 dwords, nearly always empty -- as ONE more dword a lane
// (lane l holds record dword l % 16), requested with the batch it belongs to: unconditional, the same eight loads on every
// path, so hipcc's count of the loads in flight stays exact (the decode of a batch waits with vmcnt(8), the next batch's
// eight).  Scalar loads of the record would count in lgkmcnt with the x reads from LDS: every FMA block would then wait
// for the NEXT pair's record, a round trip to memory.  deliver() decodes, then patches: one scalar compare of entry 0
// against "empty" and a skipped branch; in a pair with escapes every entry's pos and bits come out of the record dword
// with v_readlane and the thread that owns the value (pos >> 5) replaces element pos & 31 of wa / wb through a 32-way
// select -- no memory operation on that path, and no register indexed at run time.
struct PkRaw28 {
    v4u q4[7];
    uint32_t rec;
};

template <int EPI>
struct RowPacked28 {
    static constexpr int kSets = 2;
    v4f wa[kRowU], wb[kRowU];
    PkRaw28 raw[kSets];
    int e15[kSets];
    const uint32_t *pp, *pr;
    int e_pt, wave_u;

    __device__ __forceinline__ void init(const MvLocals &, int, int) { wave_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
    __device__ __forceinline__ void point(const MvLocals &m, int u)
    {
        int e;
        pp = pair_packed28<EPI>(m, u, pk28::kPairDw, pk28::kRecDw, e, pr);
        e_pt = e - 15;
    }
    template <int P>
    __device__ __forceinline__ void issue(int)
    {
        const int lane = threadIdx.x & 63;
        const uint32_t *src = pp + (size_t)wave_u * pk28::kChunkDw + lane * 4;
#pragma unroll
        for (int i = 0; i < 7; i++) raw[P].q4[i] = __builtin_nontemporal_load((const v4u *)(src + i * 256));
        // last: requested ahead of the planes it cost q|k|v 0.3 us a launch (profiles/packed28.md)
        raw[P].rec = pr[lane & (pk28::kRecDw - 1)];
        e15[P] = e_pt;
    }
    template <int P>
    __device__ __forceinline__ void deliver()
    {
        uint32_t d[pk28::kLaneDw], t[32];
#pragma unroll
        for (int i = 0; i < pk28::kLaneDw; i++) {
            const v4u v = raw[P].q4[i / 4];
            d[i] = (i % 4 == 0) ? v.x : (i % 4 == 1) ? v.y : (i % 4 == 2) ? v.z : v.w;
        }
        pk28::decode_lane_t(d, t);
        const int e = e15[P];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            wa[k] = v4f{__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k]), e), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 1]), e),
                        __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 2]), e), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 3]), e)};
            wb[k] = v4f{__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 4]), e), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 5]), e),
                        __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 6]), e), __builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 7]), e)};
        }
        const uint32_t rv = raw[P].rec;
        if (__builtin_amdgcn_readfirstlane(rv) != pk28::kNoEsc) {  // entry 0's pos: the pair has escapes (rare)
            const uint32_t tid = threadIdx.x;
#pragma unroll 1
            for (int n = 0; n < pk28::kMaxEsc; n++) {
                const uint32_t pos = __builtin_amdgcn_readlane(rv, 2 * n), bits = __builtin_amdgcn_readlane(rv, 2 * n + 1);
                if (pos == pk28::kNoEsc) break;
                const uint32_t sel = (pos >> 5) == tid ? (pos & 31u) : 32u;
                const float f = __uint_as_float(bits);
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        wa[k][j] = sel == (uint32_t)(8 * k + j) ? f : wa[k][j];
                        wb[k][j] = sel == (uint32_t)(8 * k + 4 + j) ? f : wb[k][j];
                    }
            }
        }
    }
};

#ifdef L2Z_TIMELINE
// measurement build (scripts/timeline_build.sh): wall-clock stamps (100 MHz) of every block of the row kernel, kept in
// registers and stored at the block's end.  Per (slot, block): [0] entry, [1] first weight batch requested, [2] x staged,
// [3] first unit done, [4] last unit done, [5] exit, [6] batches consumed, [7] units done
constexpr int kMtlSlots = 256, kMtlBlocks = 512;
__device__ long long g_mtl[kMtlSlots * kMtlBlocks * 8];
unsigned long long g_mtl_launches = 0;  // row-kernel launches so far: launch i stamps slot i % kMtlSlots
#define L2Z_MTL(i) tl[i] = wall_clock64()
#else
#define L2Z_MTL(i) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// Wide rows (n >= 4096, n/4 a multiple of 64: the 7B shapes): the WHOLE BLOCK works on
// one pair.  Rows 2p and 2p+1 are adjacent in memory, so a block reads one contiguous
// 8n-byte run per unit and consecutive blocks read consecutive runs -- the chip sweeps
// the matrix linearly, like a plain streaming read (DRAM page locality: +10 % over
// giving every wave its own row pair, measured).  Thread t takes float4 columns
// t, t+256, ...; per-thread component accumulators, (x+y)+(z+w), wave xor-shuffle,
// then the 4 wave partials are added in wave order.  Still a function of n only.
//
// PK = 29: the same kernel streaming the 29-bit packed copy of the weights (packed_w.h): the pair's chunks
// are read in the same (unit, batch) order, 116 instead of 128 bytes per lane and batch, and decoded into the same
// wa[] / wb[] right before the FMAs, so every sum is the fp32 kernel's bit for bit.  The raw words live in two fixed
// register sets taken in turn by a loop unrolled twice: the next batch is requested before the current one is decoded,
// no request waits on a copy of an earlier batch's words, and the decode waits for the current batch's words only.
// ---------------------------------------------------------------------------
// PK = 28: the 28-bit form of one-batch rows (RowPacked28), otherwise the same.
template <int PRO, int EPI, int XC, bool LL, int PK = 0>
__global__ __launch_bounds__(kBlock) void matvec_row_kernel(const MatvecArgs a)
{
    static_assert(PK == 0 || PK == 29 || (PK == 28 && XC == 4), "packed forms of the row kernel");
    constexpr int U = kRowU;
    using Src = typename std::conditional<PK == 28, RowPacked28<EPI>,
                                          typename std::conditional<PK == 29, RowPacked<EPI, XC>, RowF32<EPI, XC>>::type>::type;
    constexpr int NS = Src::kSets;
    extern __shared__ __attribute__((aligned(16))) float lds[];
#ifdef L2Z_TIMELINE
    long long tl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    L2Z_MTL(0);
    MvLocals m_ = mv_locals<EPI>(a);
    // packed weights are unsharded weights: no peer to push to.  Compiled out, not just never taken: the push path is a
    // loop with loads of its own, and behind it hipcc no longer counts the outstanding weight loads (vmcnt(0) again)
    if constexpr (PK != 0) m_.push = nullptr;
    const MvLocals m = m_;
    const int n4 = m.n >> 2;
    const int n_batches = (n4 + kBlock * U - 1) / (kBlock * U);
    const int n4_pad = n_batches * (kBlock * U);
    float *xs = lds;
    float *scratch = lds + 4 * n4_pad;            // kScratch floats
    float *part = scratch + kScratch;             // [2][kWaves][2] wave partials
    const v4f *xs4 = (const v4f *)xs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_units = m.n_pairs;
    const int ustride = gridDim.x;

    XStage<PRO, XC, LL> xst;
    xst.issue(a.x, a.xin, a.rms_w, n4);
    int u = blockIdx.x;  // grid <= n_units
    Src src;
    src.init(m, n4, n_batches);
    src.point(m, u);
    EpiIn ein = epi_prefetch<EPI>(m, u, tid == 0);
    EpiIn ein_next = ein;
    src.template issue<0>(0);
    L2Z_MTL(1);
    xst.finish(a.x, a.rms_w, m.n, n4_pad, xs, scratch);
    L2Z_MTL(2);

    // the request cursor: the batch the loop issues next (fp32: one past the batch in the registers; packed: one past
    // the batch in flight)
    int iu = u, ib = 0;
    bool imore = true;
    auto advance = [&]() __attribute__((always_inline)) {
        const MvStep s = mv_step(iu, ib, n_batches, ustride, n_units);
        imore = s.more;
        if (s.more) {
            if (s.unit_done) src.point(m, s.u_next);
            iu = s.u_next;
            ib = s.b_next;
        }
    };
    advance();  // past batch 0 (requested above)

    v4f acc_a = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
    ArgmaxCand best;
    int b = 0, parity = 0;
    // one (unit, batch) step on register set P; true = that was the last one.  Packed: whether the step requests a
    // further batch is decided by its caller (`ahead`), not inside -- a request under a branch that joins again before
    // the decode makes hipcc wait there for EVERY outstanding load (s_waitcnt vmcnt(0)), the batch just requested
    // included, and the decode no longer overlaps anything
    auto step = [&](auto set, auto ahead) __attribute__((always_inline)) -> bool {
        constexpr int P = decltype(set)::value;
        const MvStep s = mv_step(u, b, n_batches, ustride, n_units);
        // what the next unit's epilogue reads: with its first batch's request (fp32), or ahead of the packed requests,
        // which run further ahead (the epilogue's wait then covers no younger batch)
        auto prefetch_next = [&]() __attribute__((always_inline)) {
            if (s.more && s.unit_done) ein_next = epi_prefetch<EPI>(m, s.u_next, tid == 0);
        };
        if constexpr (NS > 1) {
            prefetch_next();
            if constexpr (decltype(ahead)::value) {
                // ffn13 alone runs faster when a wave requests the next batch only once the current one is in (one
                // batch in flight per wave, not up to two: 51.4 against 52.3 us; q|k|v the other way round, 31.5
                // against 30.6; the other kinds within noise -- profiles/packed_all_kinds.md)
                if constexpr (EPI == EPI_SWIGLU) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                src.template issue<(P + 1) % NS>(ib);
                advance();
            }
        }
        src.template deliver<P>();
#pragma unroll
        for (int k = 0; k < U; k++) {
            const v4f xv = xs4[b * (kBlock * U) + tid + kBlock * k];
            acc_a = fma4(src.wa[k], xv, acc_a);
            acc_b = fma4(src.wb[k], xv, acc_b);
        }
        if constexpr (NS == 1) {  // the next batch, the next unit's first one included
            prefetch_next();
            if (imore) {
                src.template issue<0>(ib);
                advance();
            }
        }
#ifdef L2Z_TIMELINE
        tl[6]++;
#endif
        if (s.unit_done) {
            const float sa = wave_sum(hsum4(acc_a));
            const float sb = wave_sum(hsum4(acc_b));
            float *pp_ = part + parity * (2 * kWaves);
            if (lane == 0) {
                pp_[wave] = sa;
                pp_[kWaves + wave] = sb;
            }
            __syncthreads();
            if (tid == 0) {
                const float ta = ((pp_[0] + pp_[1]) + pp_[2]) + pp_[3];
                const float tb = ((pp_[kWaves] + pp_[kWaves + 1]) + pp_[kWaves + 2]) + pp_[kWaves + 3];
                pair_epilogue<EPI>(m, u, ta, tb, true, ein);
                if (EPI == EPI_ARGMAX) {
                    const int ra_ = 2 * u, rb_ = ra_ + 1;
                    argmax_take(best, ta, ra_ + a.row_offset);
                    if (rb_ < m.total_rows) argmax_take(best, tb, rb_ + a.row_offset);
                }
            }
            ein = ein_next;
            parity ^= 1;
            acc_a = v4f{0.f, 0.f, 0.f, 0.f};
            acc_b = v4f{0.f, 0.f, 0.f, 0.f};
#ifdef L2Z_TIMELINE
            if (tl[7]++ == 0) L2Z_MTL(3);
            L2Z_MTL(4);
#endif
        }
        u = s.u_next;
        b = s.b_next;
        return !s.more;
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;
    static_assert(NS == 1 || NS == 2, "register sets of a source");
    if constexpr (NS == 1) {
        while (!step(Set0{}, std::false_type{})) {}
    } else {
        // the request cursor is one batch past the consumed one: no batch left to request = the last step
        while (true) {
            if (!imore) { step(Set0{}, std::false_type{}); break; }
            step(Set0{}, std::true_type{});
            if (!imore) { step(Set1{}, std::false_type{}); break; }
            step(Set1{}, std::true_type{});
        }
    }
    if (EPI == EPI_ARGMAX && tid == 0) {  // units ascend within a block: first index kept
        a.part_val[blockIdx.x] = best.v;
        a.part_idx[blockIdx.x] = best.i;
    }
#ifdef L2Z_TIMELINE
    L2Z_MTL(5);
    if (tid == 0 && (unsigned)a.tl_slot < (unsigned)kMtlSlots && blockIdx.x < kMtlBlocks) {
        long long *o = g_mtl + ((size_t)a.tl_slot * kMtlBlocks + blockIdx.x) * 8;
        for (int i = 0; i < 8; i++) o[i] = tl[i];
    }
#endif
}

// Generic form: any n, any alignment (the reference's 3x3 / 2x12 known-answer
// tests land here).  One pair per wave, scalar loads.
template <int PRO, int EPI>
__global__ __launch_bounds__(kBlock) void matvec_scalar_kernel(const MatvecArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MvLocals m = mv_locals<EPI>(a);
    float *xs = lds;
    float *scratch = lds + ((m.n + 3) & ~3);
    stage_x_scalar<PRO>(a.x, a.rms_w, m.n, xs, scratch);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int u = blockIdx.x * kWaves + wave; u < m.n_pairs; u += gridDim.x * kWaves) {
        const float *pa, *pb;
        pair_rows<EPI>(m, u, pa, pb);
        float sa, sb;
        dot2_scalar(pa, pb, xs, m.n, sa, sb);
        pair_epilogue<EPI>(m, u, sa, sb, lane == 0, epi_prefetch<EPI>(m, u, lane == 0));
    }
}

// lanes per pair for a row of n4 float4: the smallest power of two that puts a
// whole row in one batch of 6 loads per lane, clamped to [8, 64].  A function of
// n only (see the kernel header).
int lpr_for(int n4)
{
    int l = 8;
    while (l < 64 && l * 6 < n4) l <<= 1;
    return l;
}

struct MvLaunch {
    const void *fn;
    int lpr, u;
};

template <int PRO, int EPI, int LPR, int XC, bool LL>
MvLaunch mv_entry()
{
    return {reinterpret_cast<const void *>(&matvec_kernel<PRO, EPI, LPR, XC, LL>), LPR, MvGeom<LPR>::U};
}

template <int PRO, int EPI, bool LL>
MvLaunch mv_pick(int lpr, bool big_x)
{
    if (lpr == 8) return mv_entry<PRO, EPI, 8, 4, LL>();
    if (lpr == 16) return mv_entry<PRO, EPI, 16, 4, LL>();
    if (lpr == 32) return mv_entry<PRO, EPI, 32, 4, LL>();
    return big_x ? mv_entry<PRO, EPI, 64, 12, LL>() : mv_entry<PRO, EPI, 64, 4, LL>();
}

template <int PRO, int EPI, bool LL, int PK = 0>
const void *mv_row_fn(bool big_x)
{
    return big_x ? reinterpret_cast<const void *>(&matvec_row_kernel<PRO, EPI, 12, LL, PK>)
                 : reinterpret_cast<const void *>(&matvec_row_kernel<PRO, EPI, 4, LL, PK>);
}

// The (prologue, epilogue) pairs that exist, and in which further forms: LL = x read as LL words from the landing slot
// (sharded runs: only the pairs the forward pass launches on a gathered vector; EPI_ARGMAX there is a shard's classifier,
// the candidate exchange of greedy steps), SCALAR = the generic kernel (it has no fused-argmax epilogue), PACKED = the row
// kernel on the 29-bit copy: the decode's five row launches -- q|k|v, Wo and W2, ffn13, the classifier.
//                    PRO       EPI         LL SCALAR PACKED
#define L2Z_MV_COMBOS(X)                     \
    X(PRO_NONE, EPI_STORE,  0, 1, 0)         \
    X(PRO_NONE, EPI_RESID,  1, 1, 1)         \
    X(PRO_RMS,  EPI_STORE,  1, 1, 0)         \
    X(PRO_RMS,  EPI_ROPE,   1, 1, 1)         \
    X(PRO_RMS,  EPI_SWIGLU, 1, 1, 1)         \
    X(PRO_RMS,  EPI_ARGMAX, 1, 0, 1)
#define L2Z_IF_1(...) __VA_ARGS__
#define L2Z_IF_0(...)

// ... on the packed copy; the 28-bit form: rows of one batch only (n == 4096)
const void *mv_row_pick_packed(int pro, int epi, bool big_x, bool form28)
{
#define X(P, E, LL, SC, PK)                                                                   \
    L2Z_IF_##PK(if (pro == P && epi == E)                                                     \
                    return form28 ? reinterpret_cast<const void *>(&matvec_row_kernel<P, E, 4, false, 28>) \
                                  : mv_row_fn<P, E, false, 29>(big_x);)
    L2Z_MV_COMBOS(X)
#undef X
    return nullptr;
}

const void *mv_row_pick(int pro, int epi, bool big_x, bool ll)
{
#define X(P, E, LL, SC, PK)                                           \
    if (pro == P && epi == E && !ll) return mv_row_fn<P, E, false>(big_x); \
    L2Z_IF_##LL(if (pro == P && epi == E && ll) return mv_row_fn<P, E, true>(big_x);)
    L2Z_MV_COMBOS(X)
#undef X
    return nullptr;
}

MvLaunch mv_pick_pe(int pro, int epi, int lpr, bool big_x, bool vec, bool ll)
{
#define X(P, E, LL, SC, PK)                                                                \
    if (pro == P && epi == E && vec && !ll) return mv_pick<P, E, false>(lpr, big_x);       \
    L2Z_IF_##LL(if (pro == P && epi == E && vec && ll) return mv_pick<P, E, true>(lpr, big_x);) \
    L2Z_IF_##SC(if (pro == P && epi == E && !vec && !ll)                                   \
                    return MvLaunch{reinterpret_cast<const void *>(&matvec_scalar_kernel<P, E>), 0, 0};)
    L2Z_MV_COMBOS(X)
#undef X
    return {nullptr, 0, 0};
}
#undef L2Z_MV_COMBOS
#undef L2Z_IF_1
#undef L2Z_IF_0

// Pure streaming read (non-temporal float4 loads, 8 in flight per lane, sum kept out of DCE's
// reach): the rate the memory system gives a kernel that does nothing else -- the measured
// ceiling the mat-vec GB/s are quoted against beside the 8 TB/s spec (bench.py roofline).
__global__ __launch_bounds__(256) void stream_read_kernel(const v4f *__restrict__ p, size_t n4, float *out)
{
    constexpr int U = 8;
    size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256 * U;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    for (; i + 256 * (U - 1) < n4; i += stride) {
        v4f r[U];
#pragma unroll
        for (int k = 0; k < U; k++) r[k] = ldg_nt(p + i + 256 * k);
#pragma unroll
        for (int k = 0; k < U; k++) acc += r[k];
    }
    const float s = (acc.x + acc.y) + (acc.z + acc.w);
    if (s == 123.456f) out[blockIdx.x] = s;
}

}  // namespace

// upper bound over every instantiation (n4 padded to whole batches of <= 384 float4)
size_t matvec_lds_bytes(int n) { return (size_t)(4 * ((n >> 2) + 1024) + kScratch + 4 * kWaves + 4) * sizeof(float); }

int matvec_max_grid(int n_cus) { return n_cus * 8; }

// widths the vector kernels take (16-byte aligned operands assumed): every multiple of 4 floats -- a row whose
// float4 count is not a multiple of the lane count ends in a partial step (mv_load).  The rest (n % 4 != 0: the
// reference's 3x3 / 2x12 known-answer tests) goes to the generic scalar kernel, which has no fused-argmax epilogue
bool matvec_vector_width(int n) { return n > 0 && (n % 4) == 0; }

hipError_t launch_stream_read(const float *p, size_t n_floats, float *out, int n_cus, hipStream_t st)
{
    hipLaunchKernelGGL(stream_read_kernel, dim3(n_cus * 8), dim3(256), 0, st, (const v4f *)p, n_floats / 4, out);
    return hipGetLastError();
}

hipError_t launch_matvec(const MatvecArgs &a_in, int pro, int epi, int max_blocks_per_cu, int n_cus,
                         hipStream_t st, int *out_grid, bool *pushed)
{
    MatvecArgs a = a_in;
    if (max_blocks_per_cu > 8) max_blocks_per_cu = 8;
    bool vec = (a.n % 4) == 0 && aligned16(a.x) && aligned16(a.w0);
    if (a.rows1 > 0) vec = vec && aligned16(a.w1);
    if (a.rows2 > 0) vec = vec && aligned16(a.w2);
    if (pro == PRO_RMS) vec = vec && aligned16(a.rms_w);
    if (epi == EPI_SWIGLU && a.rows1 != a.rows0) return hipErrorInvalidValue;
    const int total_rows = a.rows0 + a.rows1 + a.rows2;
    const int n_pairs = (epi == EPI_SWIGLU) ? a.rows0 : (total_rows + 1) / 2;
    if (n_pairs <= 0 || a.n <= 0) return hipErrorInvalidValue;
    const int n4 = a.n >> 2;
    const int lpr = lpr_for(n4);
    if (epi == EPI_ARGMAX && (!vec || a.rows1 != 0 || a.rows2 != 0)) return hipErrorNotSupported;
    const Tunables &tn = tunables();
    const bool use_row = vec && n4 >= 1024 && (n4 % 64) == 0;
    const bool ll = a.xin.slots != nullptr;
    if (ll && !vec) return hipErrorNotSupported;  // callers ask matvec_vector_width() first
    // packed weights: the row kernel's packed form or nothing (no quiet f32 fall-back)
    if (a.pk != nullptr && (!use_row || ll || !pk::width_ok(a.n))) return hipErrorInvalidValue;
    if (a.pk != nullptr) a.push = nullptr;  // (unsharded: nothing to push to; the packed kernels have no push path)
    // the 28-bit form: with a packed copy only, rows of one batch only, and every segment in it or none
    const bool pk28_form = a.pk_rec != nullptr;
    if (pk28_form && (a.pk == nullptr || !pk28::width_ok(a.n))) return hipErrorInvalidValue;
    if (a.pk != nullptr && epi != EPI_SWIGLU &&
        ((a.rows1 > 0 && (a.pk_rec1 != nullptr) != pk28_form) || (a.rows2 > 0 && (a.pk_rec2 != nullptr) != pk28_form)))
        return hipErrorInvalidValue;
    // ... of every segment, pairs inside one slot
    if (a.pk != nullptr && epi != EPI_SWIGLU &&
        ((a.rows1 > 0 && a.pk1 == nullptr) || (a.rows2 > 0 && a.pk2 == nullptr) || a.rows0 % 2 || a.rows1 % 2 || a.rows2 % 2))
        return hipErrorInvalidValue;
    // the kernel form, with the LDS it carves (x padded to whole batches + scratch) and its units of work
    MvLaunch k = {nullptr, 0, 0};
    size_t lds;
    int n_units;
    const auto padded = [n4](int batch) { return ((n4 + batch - 1) / batch) * batch; };
    if (use_row) {  // the whole block on one pair
        k.fn = a.pk != nullptr ? mv_row_pick_packed(pro, epi, a.n > 4096, pk28_form) : mv_row_pick(pro, epi, a.n > 4096, ll);
        lds = (size_t)(4 * padded(kBlock * kRowU) + kScratch + 4 * kWaves) * sizeof(float);
        n_units = n_pairs;
    } else if (vec) {  // 64 / lpr pairs per wave
        k = mv_pick_pe(pro, epi, lpr, a.n > 4096, true, ll);
        if (k.fn == nullptr) return hipErrorInvalidValue;
        lds = (size_t)(4 * padded(k.lpr * k.u) + kScratch) * sizeof(float);
        const int rw = kWave / k.lpr;
        n_units = (n_pairs + rw - 1) / rw;
    } else {  // generic scalar kernel: a pair per wave
        k = mv_pick_pe(pro, epi, lpr, a.n > 4096, false, ll);
        lds = (size_t)(((a.n + 3) & ~3) + kScratch) * sizeof(float);
        n_units = n_pairs;
    }
    if (k.fn == nullptr) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // Grid (matvec_device.h): at most what is resident at once, the units dealt evenly.
    // The row kernel streams best with few blocks per CU in lock step (fewer concurrent DRAM
    // streams).  Measured at 7B, whole-token rate: 2 blocks/CU 219 tok/s, 1 -> 208, 3 -> 213,
    // 4-8 -> 208-211 (single launches shift against each other under the power cap, so the
    // choice is made on the whole-token rate).
    // grid_cap: several ranks sharing ONE GPU (tests): a launch must leave room for the peers'
    // kernels it may be waiting for
    const int per_cu = use_row && max_blocks_per_cu > tn.row_blocks ? tn.row_blocks : max_blocks_per_cu;
    const int resident = mv_resident_blocks(k.fn, lds, per_cu, n_cus, tn.grid_cap);
    const int grid = use_row ? mv_grid_block_units(n_units, resident) : mv_grid_wave_units(n_units, resident);
    if (out_grid) *out_grid = grid;
    // only single-segment epilogues of the vector kernels push (wo, ffn13, ffn2, classifier)
    if (!vec || epi == EPI_ROPE || a.rows2 != 0 || (epi != EPI_SWIGLU && a.rows1 != 0)) a.push = nullptr;
    if (pushed) *pushed = a.push != nullptr;
#ifdef L2Z_TIMELINE
    a.tl_slot = use_row ? (int)(g_mtl_launches++ % kMtlSlots) : -1;
#endif
    void *args[] = {&a};
    return hipLaunchKernel(k.fn, dim3(grid), dim3(kBlock), args, lds, st);
}

}  // namespace l2z

#ifdef L2Z_TIMELINE
// the stamps of all slots, and how many row-kernel launches there have been
extern "C" int l2z_matvec_timeline_dump(long long *out, unsigned long long *n_launches)
{
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(l2z::g_mtl), sizeof(long long) * l2z::kMtlSlots * l2z::kMtlBlocks * 8) != hipSuccess) return 1;
    *n_launches = l2z::g_mtl_launches;
    return 0;
}
#endif
