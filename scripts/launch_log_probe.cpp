// launch_log_probe.cpp -- every launch of the batched prompt pass, and of the decode launchers, logged WITHOUT a GPU.
//
// csrc/prefill_host.cpp is compiled into this program and driven with a fake runstate; every HIP entry point is a stub:
// __hipRegisterFunction keeps the kernels' names, hipMalloc hands out fake aligned addresses, hipLaunchKernel prints the
// kernel, grid, block and LDS bytes and, for the GEMM kernels and the split launch, every field of the kernel's argument.
// prefill_alloc, prefill_stage (single-sequence and ragged), prefill_half_b and score_chunk run for six shapes, 22 chunk
// lengths, L2Z_PF_X3 = 2, 1, 0, unsharded and ranks 0 and 1 of 2 and of 8 under both sharding schemes.  Two builds of the
// library launch the same kernels the same way if and only if their logs are equal: build this file against each tree
// (after `make` in its csrc/) and diff (profiles/prefill_launchers_refactor.md).
//
// `launch_log_probe decode` drives the decode launchers of matvec.o, attention.o and misc_kernels.o directly instead:
// launch_matvec over 11 widths x 6 row counts x every (prologue, epilogue) x one and three segments x LL on / off x
// packed or not x an unaligned x x L2Z_GRID_CAP 0 / 64, with the occupancy query answering 1, 2, 4, 8 in turn;
// launch_attention / launch_attention_split over head sizes, context lengths, forms and chunk counts; launch_argmax.
// launch_q8_matvec of q8_matvec.o over 7 widths x 6 row counts x every epilogue x group sizes 32 / 64 x one and three
// segments x the same occupancy answers.
// Every call logs its launch (or none) and its return code (profiles/decode_kernels_refactor.md, decode_pass_refactor.md).  The same program
// built with -Xarch_host -fsanitize=address,undefined on both lines is the host-side sanitizer run of those launchers.
//
//   C=llama2.zig_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC -ffp-contract=off -w -I$C -Iinclude -c scripts/launch_log_probe.cpp -o /tmp/llp.o
//   /opt/rocm/llvm/bin/clang++ /tmp/llp.o $C/prefill_gemm.o $C/prefill_skinny.o $C/prefill_panel.o $C/prefill_attention.o \
//       $C/prefill_ragged.o $C/score.o $C/tunables.o $C/matvec.o $C/attention.o $C/misc_kernels.o $C/q8_matvec.o -o scripts/launch_log_probe
//   scripts/launch_log_probe [L2Z_PF_PANEL L2Z_PF_FUSE_PLANES [L2Z_PF_X3_STREAM_MIN]] > launches.log
//   scripts/launch_log_probe decode > decode_launches.log
#include "prefill_host.cpp"
#include "prefill_common.h"
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <cxxabi.h>

static std::map<const void *, std::string> g_names;
static uintptr_t g_bump = 0x100000000ull;
static dim3 g_cfg_grid, g_cfg_block; static size_t g_cfg_shmem; static hipStream_t g_cfg_stream;
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *dev, unsigned, void *, void *, void *, void *, int *) { g_names[host] = dev; }
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) { g_cfg_grid = g; g_cfg_block = b; g_cfg_shmem = s; g_cfg_stream = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *s, hipStream_t *st) { *g = g_cfg_grid; *b = g_cfg_block; *s = g_cfg_shmem; *st = g_cfg_stream; return hipSuccess; }
hipError_t hipGetDevice(int *) { return hipErrorNoDevice; }
hipError_t hipDeviceGetAttribute(int *, hipDeviceAttribute_t, int) { return hipErrorNoDevice; }
static int g_occ = 2, g_log_attr = 0;
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int v) { if (g_log_attr) printf("  max dynamic LDS %d\n", v); return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *n, const void *, int, size_t) { *n = g_occ; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipFree(void *) { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = (void *)g_bump; g_bump += (n + 4095) / 4096 * 4096; return hipSuccess; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
hipError_t hipMemset(void *, int, size_t) { return hipSuccess; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { static char b[32]; snprintf(b, sizeof b, "hip error %d", (int)e); return b; }
hipError_t hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t lds, hipStream_t)
{
    std::string nm = g_names.count(fn) ? g_names[fn] : "?";
    int st = 0;
    char *dm = abi::__cxa_demangle(nm.c_str(), nullptr, nullptr, &st);
    std::string d = dm ? dm : nm;
    free(dm);
    printf("  launch %s grid %u %u %u block %u %u %u lds %zu\n", d.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
    if (d.find("prefill_gemm_dma") != std::string::npos || d.find("prefill_x3_stream") != std::string::npos ||
        d.find("prefill_skinny_dma") != std::string::npos) {
        const l2z::GemmArgs &a = *(const l2z::GemmArgs *)args[0];
        printf("    x %p w2 %p w %p out %p res %p P %d N %d K %d ldx %d ldo %d ldres %d pos0 %d rope %p hs %d n_scale %d\n", (void *)a.x,
               (void *)a.w2, (void *)a.w, (void *)a.out, (void *)a.res, a.P, a.N, a.K, a.ldx, a.ldo, a.ldres, a.pos0, (void *)a.rope, a.head_size, a.n_scale);
        printf("    wk %p wv %p outk %p outv %p nq %d nkv %d ldkv %d kvhs %zu ntx %d nty %d part %p cnt %p sk %d ldw %d x3 %p ldx3 %d kp %d x3_out %p kp_out %d defer %d\n",
               (void *)a.wk, (void *)a.wv, (void *)a.outk, (void *)a.outv, a.nq, a.nkv, a.ldkv, a.kv_head_stride, a.ntx, a.nty, (void *)a.sk_part,
               (void *)a.sk_cnt, a.sk, a.ldw, a.x3, a.ldx3, a.kp, a.x3_out, a.kp_out, a.defer);
    } else if (d.find("split3") != std::string::npos) {
        printf("    x %p ldx %d x3 %p kp %d P %d\n", *(void **)args[0], *(int *)args[1], *(void **)args[2], *(int *)args[3], *(int *)args[4]);
    }
    return hipSuccess;
}
}
namespace l2z {
int g_cus = 256;
void set_error(const char *f, ...) { va_list ap; va_start(ap, f); printf("  ERROR: "); vprintf(f, ap); printf("\n"); va_end(ap); }
int check_pair(const l2z_config *, const l2z_runstate *, const l2z_weights *, bool, bool) { return 0; }
int check_positions(const char *, const char *, const char *, int, int, int) { return 0; }
int check_tokens(const char *, const char *, const int32_t *, int, int, int) { return 0; }
int alloc_all(const char *, std::initializer_list<DeviceBuf> want)
{
    for (const DeviceBuf &b : want)
        if (*b.p == nullptr && b.bytes != 0) hipMalloc(b.p, b.bytes);
    return 0;
}
int comm_check(const l2z_comm *) { return 0; }
bool comm_bulk_ok(const l2z_comm *, size_t) { return true; }
hipError_t launch_bulk_unpack(const BulkArgs &, unsigned long long, int, float *, int, hipStream_t) { return hipSuccess; }
int comm_bulk_allgather(const l2z_comm *, float *, int, int, float *, int, hipStream_t) { return 0; }
int comm_bulk_allreduce(const l2z_comm *, float *, int, int, float *, float *, int, hipStream_t) { return 0; }
int comm_allgather_inplace(const l2z_comm *, float *, size_t, int, int, bool, hipStream_t) { return 0; }
}
static int pad_cols_(int n) { return n > 768 ? (n + 255) / 256 * 256 : (n + 3) / 4 * 4; }

static void run(const char *name, l2z_config c, int world, int rank, bool scheme_b, int x3)
{
    tunables_set("L2Z_PF_X3", x3);
    l2z_runstate s = {};
    s.cfg = c;
    Shard &sh = s.sh;
    const int hs = c.dim / c.n_heads;
    sh.rank = rank; sh.world = world; sh.hs = hs;
    sh.dim_loc = c.dim / world; sh.dim0 = rank * sh.dim_loc; sh.heads_loc = c.n_heads / world; sh.kvd_loc = c.n_kv_heads / world * hs;
    sh.hid_loc = c.hidden_dim / world; sh.hid0 = rank * sh.hid_loc; sh.v_loc = c.vocab_size / world; sh.v0 = rank * sh.v_loc;
    sh.scheme_b = scheme_b; sh.dimc_pad = pad_cols_(sh.dim_loc); sh.hidc_pad = pad_cols_(sh.hid_loc);
    g_bump = 0x100000000ull;
    void *p;
    hipMalloc(&p, 1 << 30); s.key_cache = (float *)p; hipMalloc(&p, 1 << 30); s.value_cache = (float *)p;
    hipMalloc(&p, 1 << 20); s.rope = (float2 *)p; hipMalloc(&p, 1 << 20); s.x = (float *)p; hipMalloc(&p, 1 << 20); s.logits = (float *)p;
    l2z_weights w = {};
    const float **ws[] = {&w.tok_emb, &w.rms_att, &w.rms_ffn, &w.rms_final, &w.wq, &w.wk, &w.wv, &w.wo, &w.w1, &w.w2, &w.wcls};
    for (const float **q : ws) { hipMalloc(&p, (size_t)1 << 31); *q = (const float *)p; }
    w.w3 = w.w1 + c.dim;
    static const int Ps[] = {8, 16, 17, 24, 32, 33, 40, 48, 49, 56, 64, 65, 96, 100, 128, 129, 160, 256, 257, 300, 512, 1024};
    for (int P : Ps) {
        printf("== %s world %d rank %d scheme_b %d x3 %d P %d\n", name, world, rank, (int)scheme_b, x3, P);
        if (prefill_alloc(&s, P) != 0) { printf("  alloc failed\n"); continue; }
        for (int l = 0; l < 2; l++) {
            if (scheme_b) { for (int h = 0; h < 2; h++) printf("  half %d -> %d\n", h, prefill_half_b(&s, &w, l, h, P, 3)); }
            else for (int k = 0; k < PF_STAGES; k++) { printf("  stage %d\n", k); int rc = prefill_stage(&s, &w, l, k, P, 3); if (rc) printf("  rc %d\n", rc); }
        }
        s.pf_pending.valid = false;
        if (world == 1 && !scheme_b) {
            RaggedChunk rg = {};
            hipMalloc(&p, 1 << 24); rg.k = (float *)p; hipMalloc(&p, 1 << 24); rg.v = (float *)p; rg.n_seq = 2; rg.n_tiles = 2; rg.seq_max = kRaggedMaxSeq;
            for (int k = 0; k < PF_STAGES; k++) { printf("  ragged stage %d\n", k); int rc = prefill_stage(&s, &w, 1, k, P, 0, &rg); if (rc) printf("  rc %d\n", rc); }
            s.pf_pending.valid = false;
            if (score_alloc(&s, P) == 0) {
                ScoreCall sc = {nullptr, nullptr, (int *)s.sc_seq};
                printf("  score -> %d\n", score_chunk(&s, &w, &sc, 0, P));
            }
        }
    }
}

// ---- the decode launchers, driven directly ----
static void decode_sweep()
{
    g_log_attr = 1;
    float *const base = (float *)0x200000000ull;  // fake, 16-byte aligned; nothing is dereferenced
    static const int ns[] = {3, 5, 64, 172, 288, 512, 768, 1376, 4096, 11008, 5632}, rows[] = {1, 2, 33, 288, 4096, 32000};
    for (int cap : {0, 64}) {
        tunables_set("L2Z_GRID_CAP", cap);
        for (int n : ns) for (int r : rows) for (int pro = 0; pro <= 1; pro++) for (int epi = 0; epi <= 4; epi++)
            for (int segs : {1, 3}) for (int ll = 0; ll <= 1; ll++) for (int pk = 0; pk <= 1; pk++) for (int mis = 0; mis <= 1; mis++)
                for (int occ : {1, 2, 4, 8}) {
                    if (mis && (ll || pk || occ != 2)) continue;  // the unaligned x: once per shape
                    g_occ = occ;
                    MatvecArgs a = {};
                    a.n = n; a.x = base + mis; a.rms_w = base + (1 << 20); a.resid = base + (2 << 20);
                    a.w0 = base + (16 << 20); a.out0 = base + (3 << 20); a.rows0 = r;
                    if (epi == EPI_SWIGLU) a.rows1 = r;
                    if (segs == 3) {
                        a.w1 = base + (64 << 20); a.out1 = base + (4 << 20); a.rows1 = epi == EPI_SWIGLU ? r : (r + 1) / 2;
                        if (epi != EPI_SWIGLU) { a.w2 = base + (96 << 20); a.out2 = base + (5 << 20); a.rows2 = (r + 1) / 2; }
                    }
                    a.pos_ptr = (const int *)(base + (6 << 20)); a.rope = (const float2 *)(base + (7 << 20)); a.head_size = 64; a.rope_segs = 2;
                    a.part_val = base + (8 << 20); a.part_idx = (int *)(base + (9 << 20));
                    a.push = (const P2pArgs *)(base + (10 << 20)); a.push_ctl = (const int *)(base + (11 << 20));
                    if (ll) { a.xin.slots = (const unsigned long long *)(base + (12 << 20)); a.xin.ctl = (int *)(base + (11 << 20)); }
                    if (pk) a.pk = (const uint32_t *)(base + (128 << 20));
                    int grid = -1; bool pushed = false;
                    printf("mv cap %d n %d rows %d pro %d epi %d segs %d ll %d pk %d mis %d occ %d\n", cap, n, r, pro, epi, segs, ll, pk, mis, occ);
                    const hipError_t e = launch_matvec(a, pro, epi, 8, g_cus, nullptr, &grid, &pushed);
                    printf("  -> %d grid %d pushed %d\n", (int)e, grid, (int)pushed);
                }
    }
    tunables_set("L2Z_GRID_CAP", 0);
    // launch_q8_matvec: widths x rows x epilogue x group size x one and three segments x the occupancy answers, and
    // max_blocks_per_cu values its own clamp treats differently
    const int8_t *const qbase = (const int8_t *)0x300000000ull;
    static const int qns[] = {64, 288, 768, 1408, 4096, 4224, 11008};
    for (int n : qns) for (int r : rows) for (int epi = 0; epi <= 4; epi++) for (int gs : {32, 64}) for (int segs : {1, 3})
        for (int occ : {1, 2, 4, 8}) for (int mb : {8, 0, 3, 9}) {
            if (mb != 8 && occ != 4) continue;  // the clamp: once per shape
            g_occ = occ;
            Q8MatvecArgs a = {};
            a.gs = gs;
            a.b.n = n; a.b.x = base; a.b.rms_w = epi == EPI_RESID ? nullptr : base + (1 << 20); a.b.resid = base + (2 << 20);
            a.q0 = qbase; a.s0 = base + (16 << 20); a.b.out0 = base + (3 << 20); a.b.rows0 = r;
            if (epi == EPI_SWIGLU) a.b.rows1 = r;
            if (segs == 3) {
                a.q1 = qbase + ((size_t)1 << 30); a.s1 = base + (64 << 20); a.b.out1 = base + (4 << 20); a.b.rows1 = epi == EPI_SWIGLU ? r : (r + 1) / 2;
                if (epi != EPI_SWIGLU) { a.q2 = qbase + ((size_t)2 << 30); a.s2 = base + (96 << 20); a.b.out2 = base + (5 << 20); a.b.rows2 = (r + 1) / 2; }
            }
            a.b.pos_ptr = (const int *)(base + (6 << 20)); a.b.rope = (const float2 *)(base + (7 << 20)); a.b.head_size = 64; a.b.rope_segs = 2;
            a.b.part_val = base + (8 << 20); a.b.part_idx = (int *)(base + (9 << 20));
            int grid = -1;
            printf("q8 n %d rows %d epi %d gs %d segs %d occ %d mb %d\n", n, r, epi, gs, segs, occ, mb);
            const hipError_t e = launch_q8_matvec(a, epi, mb, g_cus, nullptr, &grid);
            printf("  -> %d grid %d\n", (int)e, grid);
        }
    for (int hs : {11, 48, 64, 128}) for (int S : {256, 512, 1024, 2048}) for (int mis = 0; mis <= 1; mis++) {
        AttnArgs a = {};
        a.q = base + mis; a.kcache = base + (16 << 20); a.vcache = base + (64 << 20); a.xb = base + (3 << 20);
        a.pos_ptr = (const int *)(base + (6 << 20)); a.head_size = hs; a.kv_row = hs; a.kv_head = (size_t)S * hs; a.kv_mul = 1; a.seq_len = S;
        printf("attn hs %d seq_len %d mis %d: push_supported %d split_supported %d short_pos %d wide_pos %d lds %zu %zu\n", hs, S, mis,
               (int)attention_push_supported(a), (int)attention_split_supported(a), attention_short_pos(hs, S), attention_split_wide_pos(S),
               attention_lds_bytes(hs, S, true), attention_lds_bytes(hs, S, false));
        for (int form = 0; form <= 4; form++) {
            printf(" form %d\n", form);
            printf("  -> %d\n", (int)launch_attention(a, 32, nullptr, form));
        }
        if (!attention_split_supported(a)) continue;  // the callers' own guard: the split kernel has no scalar form
        for (int nch : {1, 2, 3, 8}) for (int small = 0; small <= 1; small++) {
            printf(" split nch %d small %d part_floats %zu\n", nch, small, attention_split_part_floats(32, hs, nch));
            printf("  -> %d\n", (int)launch_attention_split(a, 32, nch, base + (8 << 20), (int *)(base + (9 << 20)), nullptr, small != 0));
        }
    }
    for (int heads : {1, 6, 12, 32, 64, 300}) printf("split_chunks heads %d -> %d\n", heads, attention_split_chunks(heads, g_cus));
    for (int vocab : {1, 1000, 32000}) for (int parts : {0, 16}) {
        ArgmaxArgs a = {};
        a.logits = base; a.vocab = vocab; a.argmax_out = (int *)(base + (9 << 20));
        if (parts) { a.part_val = base + (8 << 20); a.part_idx = (int *)(base + (9 << 20)); a.n_part = parts; }
        printf("argmax vocab %d parts %d\n", vocab, parts);
        printf("  -> %d\n", (int)launch_argmax(a, nullptr));
    }
    for (int n : ns) printf("n %d: vector_width %d lds_bytes %zu\n", n, (int)matvec_vector_width(n), matvec_lds_bytes(n));
    printf("max_grid %d\n", matvec_max_grid(g_cus));
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "decode") { decode_sweep(); return 0; }
    if (argc > 2) { tunables_set("L2Z_PF_PANEL", atoi(argv[1])); tunables_set("L2Z_PF_FUSE_PLANES", atoi(argv[2])); }
    if (argc > 3) tunables_set("L2Z_PF_X3_STREAM_MIN", atoi(argv[3]));
    const l2z_config a = {2048, 5632, 2, 16, 16, 4096, 1024}, b = {4096, 11008, 2, 32, 32, 32000, 1024}, c = {288, 768, 2, 6, 6, 4096, 1024},
                     d = {768, 2048, 2, 12, 12, 32000, 1024}, e = {2048, 14336, 2, 16, 16, 4096, 1024}, f = {4096, 11008, 2, 32, 8, 32000, 1024};
    struct { const char *n; l2z_config c; } shapes[] = {{"a", a}, {"7B", b}, {"15M", c}, {"110M", d}, {"wide", e}, {"gqa", f}};
    for (auto &sp : shapes)
        for (int x3 = 2; x3 >= 0; x3--) {
            run(sp.n, sp.c, 1, 0, false, x3);
            if (sp.c.dim == 288) continue;
            for (int world : {2, 8})
                for (int rank : {0, 1}) {
                    if (sp.c.n_kv_heads % world) continue;
                    run(sp.n, sp.c, world, rank, false, x3);
                    run(sp.n, sp.c, world, rank, true, x3);
                }
        }
    return 0;
}
