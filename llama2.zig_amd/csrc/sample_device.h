// sample_device.h -- the sampler's row body: one token drawn from one row of logits by a block of 1024 threads, with the
// bits the host samplers give (llama2.zig_amd/host/llama2_host.cpp, main.zig:728-798).  Shared by l2z_sample_batch's
// kernel (sample_batch.hip: one block per row of a batch) and the last node of a sampled step graph (sample_step.hip:
// l2z_sample_run).  ONE text for both, so that "the token l2z_sample_batch draws" holds by construction.
//
// temperature > 0:
//   probs = softmax(logits / temperature)      probs_kernel's code over the same 1024 threads: l2z_probs_read's bits
//   top_p 0 or 1: sample (:728-741)            first i with coin < cdf_i, the cdf a sequential f32 sum in token order
//   otherwise:    sample_top_p (:754-798)      candidates >= (1 - p) / (n - 1), ordered by (probability descending,
//                                              token id ascending) -- a stable LSD radix sort of the candidates in
//                                              token order, as the host's; the sequential f32 cumulative sum until it
//                                              exceeds p; r = coin * cumulative; the first candidate whose cdf exceeds r
// The f32 sums run in the host's order on one chain (every lane of wave 0 computes it, identically): no tree sum can
// give the host's bits.  Every sum is kept, and because adding a non-negative float never lowers a sum, "the first
// index whose sum exceeds t" is then the count of sums that do NOT exceed t -- a parallel count, so the pick needs no
// second walk.  Counted as !(sum > t), which holds for a NaN sum too: on all-NaN probabilities (a NaN or a +inf in the
// logits, or nothing but -inf) no sum exceeds anything, the count is the whole chain, and the pick is the host's last
// index (:740), where `coin < cdf` never held either.
// temperature 0: the argmax of the logits, the same code as l2z_argmax_batch (argmax_rule.h).
#pragma once
#include "batch_decode.h"
#include "kernel_common.h"

namespace l2z {
namespace {

constexpr int kSbThreads = 1024, kSbWaves = kSbThreads / 64;
constexpr int kRadixBits = 8, kRadix = 1 << kRadixBits;
constexpr unsigned kDrop = kRadix;  // the digit of an item a pass leaves out
constexpr int kRounds = 8;          // rounds of 64 items a wave has in flight in a counting pass
constexpr int kWalk = 8192;         // values the prefix walk stages in LDS at a time

struct SampleLds {
    unsigned hist[kSbWaves][kRadix];  // per wave: digit counts, then the digit's next output rank
    unsigned tot[kRadix];
    __attribute__((aligned(16))) float walk[kWalk];
    float red[kScratch];
    unsigned ured[kSbWaves];
    float s_val[16];
    int s_idx[16];
    unsigned kept;
    int walked, over;
};

struct Item {
    unsigned d, key;
    int id;
};

template <class Op>
__device__ unsigned block_reduce_u32(SampleLds &L, unsigned v, Op op)
{
    for (int o = 32; o >= 1; o >>= 1) v = op(v, (unsigned)__shfl_xor((int)v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) L.ured[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = L.ured[0];
    for (int i = 1; i < kSbWaves; i++) t = op(t, L.ured[i]);
    return t;
}

// the lanes of `act` whose digit equals this lane's (8 ballots)
__device__ __forceinline__ unsigned long long same_digit(unsigned d, unsigned long long act)
{
    unsigned long long m = act;
#pragma unroll
    for (int bit = 0; bit < kRadixBits; bit++) {
        const unsigned long long bal = __ballot((d >> bit) & 1u);
        m &= ((d >> bit) & 1u) ? bal : ~bal;
    }
    return m;
}

// One stable counting pass over items [0, m): item i goes to rank (items of smaller digit) + (items of its digit
// before it); digit kDrop leaves it out.  Wave w takes the contiguous run [w * seg, (w + 1) * seg) in rounds of 64
// consecutive items, so the ranks a wave hands out follow the index order, and the waves' runs follow each other.
// get(i) -> Item; put(i, rank, item).  Returns the number of items kept.
template <class Get, class Put>
__device__ unsigned counting_pass(SampleLds &L, int m, Get get, Put put)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int seg = ((m + kSbWaves - 1) / kSbWaves + 63) & ~63;
    const int lo = min(m, w * seg), hi = min(m, lo + seg);
    for (int i = tid; i < kSbWaves * kRadix; i += kSbThreads) (&L.hist[0][0])[i] = 0;
    __syncthreads();
    for (int base = lo; base < hi; base += 64 * kRounds) {
        unsigned d[kRounds];
#pragma unroll
        for (int u = 0; u < kRounds; u++) {
            const int i = base + u * 64 + lane;
            d[u] = i < hi ? get(i).d : kDrop;
        }
#pragma unroll
        for (int u = 0; u < kRounds; u++) {
            const unsigned long long same = same_digit(d[u], __ballot(d[u] != kDrop));
            if (d[u] != kDrop && (same & below) == 0) L.hist[w][d[u]] += (unsigned)__popcll(same);
        }
    }
    __syncthreads();
    // ranks in (digit, wave) order: per digit over the waves, then the digits' totals scanned by wave 0
    if (tid < kRadix) {
        unsigned run = 0;
        for (int v = 0; v < kSbWaves; v++) {
            const unsigned c = L.hist[v][tid];
            L.hist[v][tid] = run;
            run += c;
        }
        L.tot[tid] = run;
    }
    __syncthreads();
    if (tid < 64) {
        const unsigned t0 = L.tot[4 * lane], t1 = L.tot[4 * lane + 1], t2 = L.tot[4 * lane + 2], t3 = L.tot[4 * lane + 3];
        const unsigned s = t0 + t1 + t2 + t3;
        unsigned incl = s;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += y;
        }
        const unsigned ex = incl - s;
        L.tot[4 * lane] = ex;
        L.tot[4 * lane + 1] = ex + t0;
        L.tot[4 * lane + 2] = ex + t0 + t1;
        L.tot[4 * lane + 3] = ex + t0 + t1 + t2;
        if (lane == 63) L.kept = incl;
    }
    __syncthreads();
    if (tid < kRadix) {
        const unsigned b = L.tot[tid];
        for (int v = 0; v < kSbWaves; v++) L.hist[v][tid] += b;
    }
    __syncthreads();
    for (int base = lo; base < hi; base += 64 * kRounds) {
        Item it[kRounds];
#pragma unroll
        for (int u = 0; u < kRounds; u++) {
            const int i = base + u * 64 + lane;
            if (i < hi) it[u] = get(i);
            else it[u].d = kDrop;
        }
#pragma unroll
        for (int u = 0; u < kRounds; u++) {
            const unsigned d = it[u].d;
            const unsigned long long same = same_digit(d, __ballot(d != kDrop));
            if (d != kDrop) {
                const unsigned r0 = L.hist[w][d];  // every lane of the group reads before its first lane writes
                if ((same & below) == 0) L.hist[w][d] = r0 + (unsigned)__popcll(same);
                put(base + u * 64 + lane, r0 + (unsigned)__popcll(same & below), it[u]);
            }
        }
    }
    __syncthreads();
    const unsigned kept = L.kept;
    __syncthreads();
    return kept;
}

// Sequential f32 prefix sums of val(0), val(1), ... -- the host's order -- into pre[], until a sum exceeds t or len
// values are summed.  The values are staged through LDS kWalk at a time; wave 0 runs the chain (all its lanes the
// same, reading by broadcast).  Returns how many sums stand in pre[] (at least up to the first one above t).
template <class Val>
__device__ int prefix_walk(SampleLds &L, int len, float t, Val val, float *pre)
{
    const int tid = threadIdx.x, lane = tid & 63;
    float cum = 0.0f;  // wave 0's running sum
    int done = 0;
    for (int c0 = 0; c0 < len; c0 += kWalk) {
        const int cl = min(kWalk, len - c0), cl64 = (cl + 63) & ~63;
        for (int j = tid; j < cl64; j += kSbThreads) L.walk[j] = j < cl ? val(c0 + j) : 0.0f;  // + 0.0f: the sum stays
        __syncthreads();
        if (tid < 64) {
            // 32 values a round; the next round's loads are in flight while this round's 32 dependent adds run (a load
            // or store between the adds would make every round wait out the LDS latency)
            const v4f *w4 = (const v4f *)L.walk;
            v4f cur[8], nxt[8];
#pragma unroll
            for (int g = 0; g < 8; g++) cur[g] = w4[g];
            int j = 0;
            bool over = false;
            while (j < cl64 && !over) {
                const int jn = j + 32 < cl64 ? j + 32 : j;  // (never past the staged values)
#pragma unroll
                for (int g = 0; g < 8; g++) nxt[g] = w4[(jn >> 2) + g];
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    cum = cum + cur[g].x;
                    cur[g].x = cum;
                    cum = cum + cur[g].y;
                    cur[g].y = cum;
                    cum = cum + cur[g].z;
                    cur[g].z = cum;
                    cum = cum + cur[g].w;
                    cur[g].w = cum;
                }
                if (lane == 0) {
#pragma unroll
                    for (int g = 0; g < 8; g++) ((v4f *)L.walk)[(j >> 2) + g] = cur[g];
                }
                j += 32;
                over = cum > t;
#pragma unroll
                for (int g = 0; g < 8; g++) cur[g] = nxt[g];
            }
            if (lane == 0) {
                L.walked = min(j, cl);
                L.over = over ? 1 : 0;
            }
        }
        __syncthreads();
        const int got = L.walked;
        const bool over = L.over != 0;
        for (int j = tid; j < got; j += kSbThreads) pre[c0 + j] = L.walk[j];
        done = c0 + got;
        __syncthreads();  // the staging area and the flags are rewritten next round; pre[] is complete
        if (over) break;
    }
    return done;
}

// how many of pre[0 .. len) do not exceed t (a NaN sum does not).  pre is non-decreasing, so when this is < len it is the
// first index above t -- or all NaN (a softmax is NaN everywhere or nowhere), and then this is len
__device__ int count_le(SampleLds &L, const float *pre, int len, float t)
{
    unsigned c = 0;
    for (int j = threadIdx.x; j < len; j += kSbThreads) c += !(pre[j] > t) ? 1u : 0u;
    return (int)block_reduce_u32(L, c, [](unsigned x, unsigned y) { return x + y; });
}

// The row's token (valid in thread 0): lg[0 .. n) drawn with (temperature, p, coin).  scratch: sample_scratch_floats(n)
// floats of this row's own; lg is not modified.  Every thread of the block calls it (it holds barriers).
__device__ int sample_row(SampleLds &L, const float *lg, const int n, const float temperature, const float p, const float coin,
                          float *scratch)
{
    const int tid = threadIdx.x;
    if (temperature == 0.0f) return block_argmax_1024(lg, n, L.s_val, L.s_idx);
    const size_t V = ((size_t)n + 63) / 64 * 64;  // sample_scratch_floats: five regions of V
    float *probs = scratch;
    unsigned *ka = (unsigned *)(probs + V), *kb = (unsigned *)(probs + 3 * V);
    int *ia = (int *)(probs + 2 * V), *ib = (int *)(probs + 4 * V);

    // :1005-1008 as probs_kernel computes it for l2z_probs_read (same division, same block_softmax, same 1024 threads)
    for (int i = tid; i < n; i += blockDim.x) probs[i] = lg[i] / temperature;
    __syncthreads();
    block_softmax(probs, n, L.red);

    if (p == 0.0f || p == 1.0f) {  // :1009-1010 sample (:728-741)
        float *pre = (float *)ka;
        const int walked = prefix_walk(L, n, coin, [&](int i) { return probs[i]; }, pre);
        const int c = count_le(L, pre, walked, coin);
        return c < walked ? c : n - 1;  // :740
    }

    // :759-770 the candidates, and the bit range they span (non-negative floats order like their bit patterns)
    const float cutoff = (1.0f - p) / ((float)n - 1.0f);
    unsigned hi_b = 0u, lo_b = 0xffffffffu;
    for (int i = tid; i < n; i += kSbThreads) {
        const float v = probs[i];
        if (v >= cutoff) {
            hi_b = max(hi_b, __float_as_uint(v));
            lo_b = min(lo_b, __float_as_uint(v));
        }
    }
    hi_b = block_reduce_u32(L, hi_b, [](unsigned x, unsigned y) { return max(x, y); });
    lo_b = block_reduce_u32(L, lo_b, [](unsigned x, unsigned y) { return min(x, y); });
    if (lo_b > hi_b)  // no candidate: the host falls back to the argmax of the probabilities
        return block_argmax_1024(probs, n, L.s_val, L.s_idx);
    // the candidates in token order as (key, id), key = hi_b - bits: ascending keys are descending probabilities
    const int m = (int)counting_pass(
        L, n,
        [&](int i) {
            const float v = probs[i];
            return Item{v >= cutoff ? 0u : kDrop, hi_b - __float_as_uint(v), i};
        },
        [&](int, unsigned r, const Item &it) {
            ka[r] = it.key;
            ia[r] = it.id;
        });
    // :774 the order: stable LSD passes over the digits the keys span; equal keys keep token order (lower id first)
    unsigned *sk = ka, *dk = kb;
    int *si = ia, *di = ib;
    for (unsigned span = hi_b - lo_b, shift = 0; span != 0; span >>= kRadixBits, shift += kRadixBits) {
        counting_pass(
            L, m,
            [&](int i) {
                const unsigned k = sk[i];
                return Item{(k >> shift) & (kRadix - 1u), k, si[i]};
            },
            [&](int, unsigned r, const Item &it) {
                dk[r] = it.key;
                di[r] = it.id;
            });
        unsigned *tk = sk; sk = dk; dk = tk;
        int *ti = si; si = di; di = ti;
    }
    // :776-786 cumulative sum until it exceeds p (the probabilities are no longer needed: their region takes the sums)
    float *pre = probs;
    const int walked = prefix_walk(L, m, p, [&](int j) { return __uint_as_float(hi_b - sk[j]); }, pre);
    const int c = count_le(L, pre, walked, p);
    const int cutoff_index = c < walked ? c : m - 1;  // :778
    const float r = coin * pre[cutoff_index];          // :789
    // :791-797 the cdf of the candidates is the same chain of sums: the first one above r, else the last candidate
    int pick = count_le(L, pre, cutoff_index + 1, r);
    if (pick > cutoff_index) pick = cutoff_index;
    return si[pick];
}

}  // namespace
}  // namespace l2z
