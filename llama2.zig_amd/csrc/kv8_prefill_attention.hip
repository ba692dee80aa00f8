// kv8_prefill_attention.hip -- the prompt attention over the int8 KV cache (kv8.h, kv8_layout.h): causal
// attention of a chunk's P queries over rows 0 .. pos0 + P - 1 of ONE sequence's int8 arrays, the chunk's own rows included
// (the scatter has run: what a query sees at key t is f32(q8) * s, the wide step's values).  Two forms; the row form is
// launch_kv8_attention over slices of the chunk, the matrix-core form is the kernel of this file.
//
// The frame is prefill_attention_flash's (prefill_attention.hip): one block per (head, 64 queries), the last query tiles
// first; eight waves = four query groups of 16 x two key parts of 32 rows of every tile; S^T and O^T on MFMA 16x16x4 f32
// (D[i][j] += A[i][k] B[k][j]; A: lane l holds A[l & 15][l >> 4], B: lane l holds B[l >> 4][l & 15], D: lane l, register r
// holds D[4 (l >> 4) + r][l & 15]):
//   S^T[kv][q]  = sum_h K[kv][h] Q[q][h]        A = K rows (LDS), B = Q (registers, loaded once)
//   O^T[d][q]  += sum_kv V[kv][d] P^T[kv][q]    A = V (LDS),      B = P^T
// with the PV product's k index over kv' = 4 k + s, so P goes from the S accumulators into it without leaving registers;
// running (m, l) per query; the two key parts merged through LDS at the end.  q stays f32: these are the F32 matrix cores.
//
// The data movement is the int8 one.  A key tile is 64 rows x head_size BYTES of K and as many of V (8 KB each at head_size
// 128, where the f32 kernel moves 32 KB), brought in by direct-to-LDS loads of 16 bytes a lane, and the tile's 64 K scales
// and 64 V scales by one 4-byte-a-lane load each (waves 0 and 1) beside it; two buffers, tile kt + 1 travels while tile kt
// is multiplied, one barrier a tile.  LDS: 2 x (2 x 64 x head_size + 512) bytes = 33 KB at head_size 128 (the merge's 34 KB
// reuses it), so the LDS leaves room for several blocks a CU; the registers allow two at head_size 64 and one at 128 (156
// VGPRs; at 128 the compiler spills, so the bound asks for no more).
// An operand is ONE dword: four consecutive h of a key row (with Q's float4 of the same h: k-set {16 T + 4 g + c}), or four
// consecutive d of a value row (four output tiles: O^T tile (DT, c) row i is d = 64 DT + 4 i + c).  It is converted exactly
// (kv8_unpack) in registers and feeds four MFMAs.  Both are ds_read_b32: a K read is 16 rows x the four dwords of one
// 16-byte granule, a V read four rows (4 g + s) x sixteen consecutive dwords.  Rows stand head_size bytes apart, 2 (head_size
// 128) or 4 (64) to a line of 64 banks, so unswizzled either read would put its rows on the same banks.  The granule a lane
// asks for is therefore permuted on the load's SOURCE address: granule (row, i) of a tile stands at (row * GPR + i) ^
// kv8_swz(row), a XOR inside the row's own 256-byte line, chosen so that both reads touch each of the 64 banks once.
// Scales, in the decode kernel's order: a score is (dot * ks[t]) / sqrt(head_size); the weight that enters the PV product is
// e * vs[t], formed once per (query, key).  A tile is loaded whole, so rows beyond a query's position ARE read (clamped to
// row seq_len - 1, never past the arrays) and their bytes and scales may be anything: the masked score and the masked V
// scale are SELECTED (live ? x : -inf, live ? vs : 0), neither is multiplied by a zero weight, and the bytes of a dead key
// meet an exactly zero weight.  Vector loads and stores only.
// The merge's rows in LDS stand 4 NDT + 2 floats apart (34 at head_size 128), a lane a row: those accesses are NOT free of
// bank conflicts.  They run once a block, after the last tile.
#include "kv8.h"

#include "kernel_common.h"
#include "kv8_device.h"
#include "kv8_layout.h"
#include "prefill_common.h"

namespace l2z {
namespace {

struct Kv8FlashArgs {
    const float *q;
    float *out;
    Kv8Seq seq;                         // layer 0's bases
    size_t layer_off, kv_head_stride;   // in values; a scale stands at (the value's index) / head_size
    int ldq, ldo, pos0, P, kv_mul, seq_len;
};

// one 4-byte-a-lane direct-to-LDS load: lane l's dword from `g` (per lane) to lds + 4 * l (`lds` wave-uniform)
__device__ __forceinline__ void lds_dma4(const float *g, float *lds)
{
    __builtin_amdgcn_global_load_lds(g, lds, 4, 0, 0);
}

// The XOR a row's granules take inside the row's line of 16 granules (= 64 banks), a function of the row's place among 16.
// head_size 128 (8 granules a row, rows r and r ^ 1 share a line): bits 1, 2, 3 of the row; 64 (4 granules, four rows a
// line): bits 2 and 3.  Rows of one line take the same XOR, so the map is a permutation of the line.
template <int HS> __device__ __forceinline__ int kv8_swz(int row)
{
    if (HS == 128) return 9 * ((row >> 2) & 1) + 4 * ((row >> 3) & 1) + 2 * ((row >> 1) & 1);
    return 5 * ((row >> 2) & 3);
}

template <int NDT>
__global__ __launch_bounds__(512, NDT == 4 ? 4 : 2) void kv8_prefill_flash(const Kv8FlashArgs a)
{
    constexpr int HS = 16 * NDT, GPR = HS / 16;   // 16-byte granules a row
    constexpr int TILE = 64 * HS;                 // bytes of a K tile, and of a V tile
    constexpr int BUF = 2 * TILE + 2 * 64 * 4;    // K | V | the K scales | the V scales
    constexpr int LPW = 2 * NDT / 8;              // wave-wide 1-KB loads per wave and tile (K and V together: 2 NDT)
    static_assert(NDT == 4 || NDT == 8, "head_size 64 or 128");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    // blocks are dispatched in id order: the query tiles with the most key tiles (the LAST queries) first
    const int h = blockIdx.x, q0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qg = wave & 3, kh = wave >> 2;  // query group (16 queries), key part (rows 32 kh .. of a tile)
    const int qi = lane & 15, g = lane >> 4;
    const int kvh = h / a.kv_mul;
    const size_t head_off = a.layer_off + (size_t)kvh * a.kv_head_stride;
    const int8_t *kbase = a.seq.k8 + head_off, *vbase = a.seq.v8 + head_off;
    const float *ksbase = a.seq.ks + head_off / (size_t)HS, *vsbase = a.seq.vs + head_off / (size_t)HS;
    const int P = a.P, pos0 = a.pos0, seq_len = a.seq_len;
    const int myq = q0 + 16 * qg + qi;              // this lane's query (row of the chunk)
    const int qrow = myq < P ? myq : P - 1;         // past the chunk: the last row once more, results dropped
    const int mypos = pos0 + qrow;
    v4f qreg[NDT];
#pragma unroll
    for (int T = 0; T < NDT; T++) qreg[T] = *(const v4f *)(a.q + (size_t)qrow * a.ldq + (size_t)h * HS + 16 * T + 4 * g);
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    v4f ot[NDT];
#pragma unroll
    for (int d = 0; d < NDT; d++) ot[d] = zero;
    float m = -INFINITY, lsum = 0.0f;
    const int last_q = (q0 + 63 < P ? q0 + 63 : P - 1);
    const int n_kt = (pos0 + last_q) / 64 + 1;              // key tiles of the block
    const int last_live = pos0 + q0 + 16 * qg + 15;         // last key position live for one of this wave's queries
    const float div = sqrtf((float)HS);
    auto issue = [&](int kt, int buf) {
        const int t0 = kt * 64;
        unsigned char *kd = lds8 + buf * BUF;
#pragma unroll
        for (int i = 0; i < LPW; i++) {
            const int j = wave + 8 * i;                     // K's loads 0 .. NDT - 1, then V's (wave-uniform)
            const bool is_v = j >= NDT;
            const int ld = is_v ? j - NDT : j;
            const int p = ld * 64 + lane;                   // the granule's place in the tile
            const int at = p ^ kv8_swz<HS>((p >> 4) * (16 / GPR));   // ... holds this (row, granule)
            int t = t0 + at / GPR;
            t = t < seq_len ? t : seq_len - 1;              // rows past the context are masked below
            const int8_t *src = (is_v ? vbase : kbase) + (size_t)t * HS + 16 * (at % GPR);
            lds_dma16((const float *)src, (float *)(kd + (is_v ? TILE : 0) + ld * 1024));
        }
        if (wave < 2) {                                     // the tile's 64 K scales, its 64 V scales
            int t = t0 + lane;
            t = t < seq_len ? t : seq_len - 1;
            lds_dma4((wave == 0 ? ksbase : vsbase) + t, (float *)(kd + 2 * TILE) + 64 * wave);
        }
    };
    const int swz_k = kv8_swz<HS>(qi);
    issue(0, 0);
    for (int kt = 0; kt < n_kt; kt++) {
        const int t0 = kt * 64;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of tile kt has landed
        __syncthreads();  // everyone's has; and every wave is done with tile kt - 1: its buffer is free
        if (kt + 1 < n_kt) issue(kt + 1, (kt + 1) & 1);
        const int *kb = (const int *)(lds8 + (kt & 1) * BUF), *vb = kb + TILE / 4;
        const float *ksb = (const float *)(vb + TILE / 4), *vsb = ksb + 64;
        const int r0 = 32 * kh;                        // this wave's rows of the tile: r0 .. r0 + 31
        if (t0 + r0 > last_live) continue;             // nothing live for this wave (wave-uniform)
        v4f st[2] = {zero, zero};
#pragma unroll
        for (int T = 0; T < NDT; T++)  // the two accumulators interleaved: independent MFMA chains
#pragma unroll
            for (int jt = 0; jt < 2; jt++) {
                const int row = r0 + 16 * jt + qi;
                const v4f kf = kv8_unpack(kb[4 * ((row * GPR + T) ^ swz_k) + g]);
#pragma unroll
                for (int c = 0; c < 4; c++)
                    st[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c], qreg[T][c], st[jt], 0, 0, 0);
            }
        // st[jt][r] = (q . k8)[key t0 + r0 + 16 jt + 4 g + r][query myq]: the key's scale, 1 / sqrt(head_size), causal mask
        float mx = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
            const v4f ksc = *(const v4f *)(ksb + r0 + 16 * jt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool live = t0 + r0 + 16 * jt + 4 * g + r <= mypos;  // t <= pos of the query
                st[jt][r] = live ? (st[jt][r] * ksc[r]) / div : -INFINITY;
                mx = fmaxf(mx, st[jt][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        // a query none of whose keys this wave has seen live yet (the upper key part of the first tiles): every weight is
        // e^(-inf) = 0 against any finite reference
        const float mref = m_new == -INFINITY ? 0.0f : m_new;
        float sum = 0.0f;
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
            const v4f vsc = *(const v4f *)(vsb + r0 + 16 * jt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool live = t0 + r0 + 16 * jt + 4 * g + r <= mypos;
                const float e = expf(st[jt][r] - mref);
                sum += e;
                st[jt][r] = e * (live ? vsc[r] : 0.0f);   // the weight of the PV product, once per (query, key)
            }
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float alpha = expf(m - mref);  // first live tile: e^(-inf) = 0
        lsum = lsum * alpha + sum;
        m = m_new;
#pragma unroll
        for (int d = 0; d < NDT; d++) ot[d] *= alpha;
        // O^T += V8^T (P vs)^T, k index of step (jt, s) = key rows r0 + 16 jt + 4 k + s
#pragma unroll
        for (int DT = 0; DT < NDT / 4; DT++)
#pragma unroll
            for (int jt = 0; jt < 2; jt++)
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const int row = r0 + 16 * jt + 4 * g + s4;
                    const v4f vf = kv8_unpack(vb[4 * ((row * GPR + 4 * DT + (qi >> 2)) ^ kv8_swz<HS>(4 * g + s4)) + (qi & 3)]);
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        ot[4 * DT + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[c], st[jt][s4], ot[4 * DT + c], 0, 0, 0);
                }
    }
    // the two key parts of a query group: merge (m, l, O) of the upper part into the lower one, both rescaled to the
    // common maximum
    __syncthreads();  // the buffers are free
    float *mg = (float *)lds8 + (size_t)(qg * 64 + lane) * (4 * NDT + 2);
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
    // ot[4 DT + c][r] = O^T[d = 64 DT + 16 g + 4 r + c][query myq]: 16 consecutive d per (lane, DT)
    if (myq < P) {
        float *o = a.out + (size_t)myq * a.ldo + (size_t)h * HS;
#pragma unroll
        for (int DT = 0; DT < NDT / 4; DT++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                v4f v;
#pragma unroll
                for (int c = 0; c < 4; c++) v[c] = ot[4 * DT + c][r] / lsum;
                *(v4f *)(o + 64 * DT + 16 * g + 4 * r) = v;
            }
    }
}

template <int NDT> constexpr size_t kv8_flash_lds()
{
    constexpr size_t tiles = 2 * (2 * 64 * 16 * NDT + 2 * 64 * 4), merge = (size_t)256 * (4 * NDT + 2) * 4;
    return tiles > merge ? tiles : merge;
}

}  // namespace

bool kv8_prefill_flash_shape(int head_size, int P)
{
    return (head_size == 64 || head_size == 128) && P > 32;
}

hipError_t launch_kv8_prefill_attention(const float *q, int ldq, const Kv8Prompt &seq8, float *out, int ldo, int pos0, int P,
                                        int n_heads, int head_size, int kv_mul, int seq_len, size_t layer_off, size_t kv_head_stride,
                                        hipStream_t st, int form)
{
    const int hs = head_size;
    if (q == nullptr || out == nullptr || P < 1 || pos0 < 0 || pos0 + P > seq_len || !kv8::head_size_ok(hs) || n_heads < 1 || kv_mul < 1 ||
        n_heads % kv_mul != 0 || (ldq & 3) || (ldo & 3) || (((uintptr_t)q | (uintptr_t)out) & 15) || (form != 0 && form != 1 && form != 3) ||
        kv_head_stride != (size_t)seq_len * hs || layer_off % kv_head_stride != 0 || seq8.seq.k8 == nullptr || seq8.seq.v8 == nullptr ||
        seq8.seq.ks == nullptr || seq8.seq.vs == nullptr)
        return hipErrorInvalidValue;
    const bool flash = kv8_prefill_flash_shape(hs, P);
    if (form == 3 && !flash) return hipErrorInvalidValue;
    if (flash && form != 1) {
        if ((((uintptr_t)seq8.seq.k8 | (uintptr_t)seq8.seq.v8) & 15) || (((uintptr_t)seq8.seq.ks | (uintptr_t)seq8.seq.vs) & 3))
            return hipErrorInvalidValue;
        Kv8FlashArgs a = {};
        a.q = q; a.out = out; a.seq = seq8.seq;
        a.layer_off = layer_off; a.kv_head_stride = kv_head_stride;
        a.ldq = ldq; a.ldo = ldo; a.pos0 = pos0; a.P = P; a.kv_mul = kv_mul; a.seq_len = seq_len;
        const dim3 grid(n_heads, (P + 63) / 64);
        if (hs == 128) hipLaunchKernelGGL(kv8_prefill_flash<8>, grid, dim3(512), kv8_flash_lds<8>(), st, a);
        else hipLaunchKernelGGL(kv8_prefill_flash<4>, grid, dim3(512), kv8_flash_lds<4>(), st, a);
        return hipGetLastError();
    }
    // the row form: the chunk's rows through the wide step's launches, at most kWideMax rows a launch; slice i's table names
    // the positions pos0 + kWideMax i .., every slot the one sequence
    if (seq8.tab == nullptr || seq8.slots == nullptr || seq8.part == nullptr) return hipErrorInvalidValue;
    for (int r = 0, i = 0; r < P; r += kWideMax, i++) {
        const int rows = P - r < kWideMax ? P - r : kWideMax;
        const WideAttn wa = {seq8.tab + i, seq8.part, seq8.seg_cap, (pos0 + r + rows - 1) / kVerifySeg + 1, 0, rows, 0};
        const RaggedLayer L = {q + (size_t)r * ldq, ldq, out + (size_t)r * ldo, ldo, rows, n_heads, hs, kv_mul, seq_len,
                               layer_off, kv_head_stride, st, nullptr, 0};
        const hipError_t e = launch_kv8_attention(L, wa, seq8.slots);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace l2z
