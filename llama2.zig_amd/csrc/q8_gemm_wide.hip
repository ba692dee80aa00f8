// q8_gemm_wide.hip -- the register-blocked form of the GEMM on int8 group-quantized weights for 17 .. 128 token rows
// (DESIGN.md 4.27): the product of the wide step l2z_transformer_wide_q8.  Compiled with -ffp-contract=off like every kernel
// file, and with the packed f32 instructions off (Makefile): every statement on four sums is four scalar-lane operations,
// and the group size 64 / NT = 4 kernels fit 256 registers without scratch only so (the Makefile rule fails on scratch).
//
// THE ARITHMETIC is q8_gemm_device.h's, term by term: one MFMA into a zeroed tile a group (Q8Frag), (f32(I) * ws) * xs fused
// into the lane's sum in increasing group order, wave w of eight takes groups w, w + 8, ..., a wave's groups go in batches of
// kQgBatch with the groups past the row end multiplied as zero fragments against group 0 -- q8_gemm_wave_sums' batches, so
// the +0 terms stand where its do --, the eight waves' sums added in wave order (q8_gemm_stash, q8_gemm_tile_sum).  The bits
// of a (token row, weight row) product are launch_q8_gemm's.
//
// THE BLOCKING is what differs.  q8_gemm_kernel's wave owns ONE 16-row weight tile: for each group it loads one weight
// fragment and one token fragment per MFMA, about 1 KB of operand an MFMA out of L2.  Here a block owns kQwRT = 2
// consecutive weight tiles and EVERY token tile of the call (m <= 128: at most eight), NT = 2 or 4 of them a pass.  For a
// group a wave loads kQwRT weight fragments with their scales and the pass's NT token fragments with theirs, once each, and
// issues kQwRT x NT MFMAs from registers: (kQwRT + NT) / (kQwRT NT) KB an MFMA, 0.75 KB at NT = 4.  The sums are
// 4 kQwRT NT registers a lane (32 at NT = 4), the hand-over 8 kQwRT NT KB of LDS (64 KB), one round a pass.  Up to 64 rows a
// call is one pass; beyond, a block reads its 32 weight rows once more.  (Eight token tiles a pass, or four weight tiles a
// block, spill: the compiler's report shows scratch at 256 registers for either.)  The loads of a batch's groups -- all four
// at NT = 2, two and two at NT = 4 -- are requested before the first MFMA waits, and the loop is straight-line: a tile
// past the call's last is the pass's first again, a weight row past the matrix a zero fragment at row 0's address, and
// neither is stored.  No atomics.
#include "q8_gemm_device.h"

namespace l2z {
namespace {

constexpr int kQwRT = 2;       // weight-row tiles of a block
constexpr int kQwMinRows = 17, kQwMaxRows = 128;

template <int EPI, int GS, int RT, int NT>
__global__ __launch_bounds__(kQgBlock) void q8_gemm_wide_kernel(const Q8GemmArgs a)
{
    typedef typename Q8Frag<GS>::T Frag;
    constexpr int LB = GS / 4;                      // bytes of a group a lane holds
    constexpr int TT = RT * NT;                     // a pass's (weight tile, token tile) pairs: pair r * NT + j
    constexpr int SB = TT > 4 ? 2 : kQgBatch;       // groups whose loads are in flight together
    __shared__ v4f part[kQgWaves * TT * kWave];
    // (the wave index as a scalar: with it the group index and every base address below are scalar too)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int n = a.n, ng = n / GS;
    const int n_tiles = (a.m + kQ8GemmTile - 1) / kQ8GemmTile;   // token tiles of the call (block-uniform)
    const int row0 = blockIdx.x * (RT * 16);
    // Every load is a block-uniform base -- the group's and the tile's place -- plus a 32-bit offset of the lane (the
    // launcher holds both matrices under 4 GiB).
    // A: weight row row0 + 16 r + col of tile r (past the matrix: zeros); its four output rows' scales: rows row0 + 16 r +
    // 4 quad + i, all in the matrix or none (d is a multiple of 4)
    unsigned a_off[RT], s_off[RT];
    bool a_in[RT];
#pragma unroll
    for (int r = 0; r < RT; r++) {
        const int a_row = row0 + 16 * r + col, o_row = row0 + 16 * r + 4 * quad;
        a_in[r] = a_row < a.d;
        a_off[r] = (unsigned)(a_in[r] ? a_row : 0) * (unsigned)n + quad * LB;
        s_off[r] = (unsigned)(o_row < a.d ? o_row : 0) * (unsigned)ng;
    }
    // B: token row 16 j + col of tile j (the rows stand padded to whole tiles), and its scales
    const unsigned b_off = (unsigned)col * (unsigned)n + quad * LB, x_off = (unsigned)col * (unsigned)ng;

    // A pass: NT token tiles from tile0 on against the block's RT weight tiles, over the whole of K, then the hand-over.
    // Up to 64 rows that is the call; beyond, the block's weight rows are read once more (non-temporal again: whether that
    // read is served on the die has not been measured), and a call of 65 .. 80 rows spends RT x NT MFMAs a group on one tile.
    for (int tile0 = 0; tile0 < n_tiles; tile0 += NT) {
        const int nt = n_tiles - tile0 < NT ? n_tiles - tile0 : NT;   // (block-uniform)
        v4f acc[TT];
#pragma unroll
        for (int t = 0; t < TT; t++) acc[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        for (int g0 = wave; g0 < ng; g0 += kQgWaves * kQgBatch) {
#pragma unroll
            for (int u0 = 0; u0 < kQgBatch; u0 += SB) {
                Frag wa[SB][RT], xb[SB][NT];
                v4f wsc[SB][RT];
                float xs[SB][NT];
#pragma unroll
                for (int u = 0; u < SB; u++) {
                    const int g = g0 + kQgWaves * (u0 + u);
                    const bool in = g < ng;  // (wave-uniform)
                    const int gg = in ? g : 0;
                    const int8_t *wg = a.wq + (size_t)gg * GS;
                    const float *sg = a.ws + gg;
#pragma unroll
                    for (int r = 0; r < RT; r++) {
                        wa[u][r] = (in && a_in[r]) ? __builtin_nontemporal_load((const Frag *)(wg + a_off[r])) : Q8Frag<GS>::zero();
                        wsc[u][r] = v4f{sg[s_off[r]], (sg + ng)[s_off[r]], (sg + 2 * ng)[s_off[r]], (sg + 3 * ng)[s_off[r]]};
                    }
#pragma unroll
                    for (int j = 0; j < NT; j++) {
                        const int jj = tile0 + (j < nt ? j : 0);
                        xb[u][j] = *(const Frag *)(a.xq + ((size_t)jj * kQ8GemmTile * (size_t)n + (size_t)gg * GS) + b_off);
                        xs[u][j] = (a.xs + ((size_t)jj * kQ8GemmTile * (size_t)ng + gg))[x_off];
                    }
                }
                // RT x NT MFMAs a group from registers; a pair's terms arrive in increasing group order
#pragma unroll
                for (int u = 0; u < SB; u++)
#pragma unroll
                    for (int r = 0; r < RT; r++)
#pragma unroll
                        for (int j = 0; j < NT; j++) {
                            const v4i I = Q8Frag<GS>::mfma(wa[u][r], xb[u][j]);
                            const v4f p = v4f{(float)I.x, (float)I.y, (float)I.z, (float)I.w} * wsc[u][r];
                            acc[r * NT + j] = __builtin_elementwise_fma(p, v4f{xs[u][j], xs[u][j], xs[u][j], xs[u][j]}, acc[r * NT + j]);
                        }
            }
        }
        // the K ranges' sums of a pair, added in wave order by the wave that stores the pair
        if (tile0 != 0) __syncthreads();   // (the pass before has read its sums)
        q8_gemm_stash<TT>(part, acc, wave, lane);
        for (int t = wave; t < TT; t += kQgWaves) {
            const int r = t / NT, j = t % NT;
            const int o_row = row0 + 16 * r + 4 * quad, tok = (tile0 + j) * kQ8GemmTile + col;
            if (j >= nt) continue;
            v4f v = q8_gemm_tile_sum<TT>(part, t, lane);
            if (tok >= a.m || o_row >= a.d) continue;
            if (EPI == EPI_SWIGLU) {  // rows 2p, 2p + 1 = W1 row p, W3 row p: two gated values (main.zig:411-416)
                v2f h;
                h.x = v.x * (1.0f / (1.0f + expf(-v.x)));
                h.x = h.x * v.y;
                h.y = v.z * (1.0f / (1.0f + expf(-v.z)));
                h.y = h.y * v.w;
                *(v2f *)(a.out + (size_t)tok * (size_t)a.ldo + (o_row >> 1)) = h;
            } else {
                if (EPI == EPI_RESID) v = *(const v4f *)(a.res + (size_t)tok * (size_t)a.ldres + o_row) + v;  // :395 / :422
                *(v4f *)(a.out + (size_t)tok * (size_t)a.ldo + o_row) = v;
            }
        }
    }
}

template <int GS, int RT, int NT>
const void *q8_gemm_wide_pick(int epi)
{
    switch (epi) {
        case EPI_STORE: return reinterpret_cast<const void *>(&q8_gemm_wide_kernel<EPI_STORE, GS, RT, NT>);
        case EPI_RESID: return reinterpret_cast<const void *>(&q8_gemm_wide_kernel<EPI_RESID, GS, RT, NT>);
        case EPI_SWIGLU: return reinterpret_cast<const void *>(&q8_gemm_wide_kernel<EPI_SWIGLU, GS, RT, NT>);
        default: return nullptr;
    }
}

template <int GS>
const void *q8_gemm_wide_pick_nt(int epi, int nt)
{
    return nt == 2 ? q8_gemm_wide_pick<GS, kQwRT, 2>(epi) : q8_gemm_wide_pick<GS, kQwRT, 4>(epi);
}

}  // namespace

hipError_t launch_q8_gemm_wide(const Q8GemmArgs &a, int epi, hipStream_t st)
{
    if ((a.gs != 32 && a.gs != 64) || a.m < kQwMinRows || a.m > kQwMaxRows || a.n <= 0 || a.n % a.gs != 0 || a.d <= 0 || (a.d & 3) != 0)
        return hipErrorInvalidValue;
    if (a.xq == nullptr || a.xs == nullptr || a.wq == nullptr || a.ws == nullptr || a.out == nullptr) return hipErrorInvalidValue;
    // launch_q8_gemm's alignment rules: 16-byte loads of both operands' rows, 16-byte stores of four features (SwiGLU: 8 of two)
    if (!aligned16(a.xq) || !aligned16(a.wq) || !aligned16(a.out) || (a.ldo & 3) != 0 || a.ldo < (epi == EPI_SWIGLU ? a.d / 2 : a.d))
        return hipErrorInvalidValue;
    if (epi == EPI_RESID && (a.res == nullptr || !aligned16(a.res) || (a.ldres & 3) != 0 || a.ldres < a.d)) return hipErrorInvalidValue;
    // (a lane's place in either matrix is a 32-bit offset)
    if ((unsigned long long)a.d * (unsigned long long)a.n > 0xffffffffULL) return hipErrorInvalidValue;
    // every token tile of the call in one block: two a pass for up to 32 rows, else four
    const int n_tiles = (a.m + kQ8GemmTile - 1) / kQ8GemmTile;
    const int nt = n_tiles <= 2 ? 2 : 4;
    const void *fn = a.gs == 32 ? q8_gemm_wide_pick_nt<32>(epi, nt) : q8_gemm_wide_pick_nt<64>(epi, nt);
    if (fn == nullptr) return hipErrorInvalidValue;
    const int blocks = ((a.d + 15) / 16 + kQwRT - 1) / kQwRT;
    Q8GemmArgs args = a;
    void *params[] = {&args};
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kQgBlock), params, 0, st);
}

}  // namespace l2z
