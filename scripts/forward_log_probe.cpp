// forward_log_probe.cpp -- every launch of the single-sequence decode pass, logged WITHOUT a GPU.
//
// csrc/forward.cpp is compiled into this program and enqueue_forward is driven over a fake runstate and fake weights;
// HIP and every launcher forward.cpp calls are stubs.  A launcher's stub prints its name, the prologue / epilogue and
// EVERY field of its argument block, and answers out_grid and pushed deterministically; the event calls of the per-kind
// profile print too, so the accounting around a launch is part of the log.  (comm_allgather_inplace with a null
// communicator prints nothing: the real one does nothing there.)  Three shapes -- GQA, an MHA shape whose runstate takes
// the one-launch q|k|v + attention form, the 7B widths with 2 layers -- each with f32 weights without a packed copy,
// every kind packed at 29 bits, ffn13 and cls at 28 bits, a q|k|v layer with only two slots packed, the packed-kinds
// masks 0 / each single bit / all, int8 weights at group sizes 32 and 64, the three step kinds, the four attention
// variants, only_kind -1 and each kind, with and without the profile; then ranks 0 and 1 of 2 under both sharding
// schemes with only_stage over all stages (emulated ranks), the same ranks on the peer-write transport in its forms, and
// the refusals of int8 weights there.  Only fields that the trees being compared both have are filled.
//
// Two builds of the library enqueue the same pass if and only if their logs are equal: build this file against each tree
// and compare (profiles/decode_pass_refactor.md).  Built with -Xarch_host -fsanitize=address,undefined it is the
// host-side sanitizer run of the walk.
//
//   C=llama2.zig_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC -ffp-contract=off -w -I$C -Iinclude -c scripts/forward_log_probe.cpp -o /tmp/flp.o
//   /opt/rocm/llvm/bin/clang++ /tmp/flp.o -o scripts/forward_log_probe
//   scripts/forward_log_probe > forward.log
#include "forward.cpp"
#include <cstdarg>
#include <cstdio>

#define P(x) ((void *)(x))
static uintptr_t g_ev = 0x10;
extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)(g_ev += 0x10); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) { printf("  event %p stream %p\n", P(e), P(st)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { static char b[32]; snprintf(b, sizeof b, "hip error %d", (int)e); return b; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t *, hipGraph_t, hipGraphNode_t *, char *, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipHostMalloc(void **, size_t, unsigned) { return hipErrorNotSupported; }
hipError_t hipMalloc(void **, size_t) { return hipErrorNotSupported; }
hipError_t hipMemcpy(void *, const void *, size_t, hipMemcpyKind) { return hipSuccess; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
hipError_t hipMemset(void *, int, size_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *) { return hipErrorNotSupported; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
const char *l2z_last_error(void) { return ""; }
}

static void print_mv(const MatvecArgs &a)
{
    printf("    w %p %p %p out %p %p %p rows %d %d %d pos_stride %d %d kvhs %zu n %d x %p rms_w %p resid %p pos_ptr %p rope %p hs %d rope_segs %d\n",
           P(a.w0), P(a.w1), P(a.w2), P(a.out0), P(a.out1), P(a.out2), a.rows0, a.rows1, a.rows2, a.pos_stride1, a.pos_stride2,
           a.kv_head_stride, a.n, P(a.x), P(a.rms_w), P(a.resid), P(a.pos_ptr), P(a.rope), a.head_size, a.rope_segs);
    printf("    part %p %p row_offset %d push %p ctl %p gi %d xin %p %u %u %d %p %p %lld pk %p %p %p e %d %d %d rec %p %p %p tl_slot %d\n",
           P(a.part_val), P(a.part_idx), a.row_offset, P(a.push), P(a.push_ctl), a.push_gi, P(a.xin.slots), a.xin.slot_floats,
           a.xin.count, a.xin.gi, P(a.xin.ctl), P(a.xin.h_err), a.xin.timeout_ticks, P(a.pk), P(a.pk1), P(a.pk2), a.pk_e, a.pk_e1,
           a.pk_e2, P(a.pk_rec), P(a.pk_rec1), P(a.pk_rec2), a.tl_slot);
}
static void print_attn(const AttnArgs &a)
{
    printf("    q %p k %p v %p xb %p pos_ptr %p hs %d kv_row %d kv_head %zu kv_mul %d seq_len %d push %p ctl %p gi %d tl_seq %d\n", P(a.q),
           P(a.kcache), P(a.vcache), P(a.xb), P(a.pos_ptr), a.head_size, a.kv_row, a.kv_head, a.kv_mul, a.seq_len, P(a.push),
           P(a.push_ctl), a.push_gi, a.tl_seq);
}

namespace l2z {
int g_cus = 256;
void set_error(const char *f, ...) { va_list ap; va_start(ap, f); printf("  ERROR: "); vprintf(f, ap); printf("\n"); va_end(ap); }
int check_draw(const char *, int, float, float, const float *) { return 0; }
int check_coins(const char *, const float *, int, int, int) { return 0; }
int no_device_check() { return 0; }
int comm_check(const l2z_comm *) { return 0; }
bool prefill_enabled() { return false; }
bool prefill_usable(const l2z_runstate *) { return false; }
int prefill_tokens(l2z_runstate *, const l2z_weights *, const int32_t *, int, int, const ScoreCall *) { return 0; }
hipError_t launch_probs(float *, const float *, int, float, hipStream_t) { return hipSuccess; }
hipError_t launch_sum_parts(float *, const float *const *, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_set_state(int token, int pos, int *tp, int *pp, const float *emb, float *x, int dim, hipStream_t st)
{
    printf("  launch_set_state %d %d %p %p %p %p %d %p\n", token, pos, P(tp), P(pp), P(emb), P(x), dim, P(st));
    return hipSuccess;
}
hipError_t launch_set_state_q8(int token, int pos, int *tp, int *pp, const Q8Emb &e, float *x, int dim, hipStream_t st)
{
    printf("  launch_set_state_q8 %d %d %p %p emb %p %p %d %p %d %p\n", token, pos, P(tp), P(pp), P(e.q), P(e.s), e.gs, P(x), dim, P(st));
    return hipSuccess;
}
bool matvec_vector_width(int n) { return n > 0 && n % 4 == 0; }
bool attention_push_supported(const AttnArgs &a) { return a.head_size % 4 == 0; }
bool attention_split_supported(const AttnArgs &a) { return a.head_size % 4 == 0; }
LLIn comm_ll_in(const l2z_comm *c, int gi, size_t count)
{
    printf("  comm_ll_in rank %d of %d gi %d count %zu\n", c->rank, c->world, gi, count);
    LLIn in = {};
    in.slots = (const unsigned long long *)(c->arena + kP2pFlagBytes);
    in.slot_floats = (unsigned)c->slot_floats; in.count = (unsigned)count; in.gi = comm_gi(c, gi);
    in.ctl = c->d_ctl; in.h_err = c->h_err; in.timeout_ticks = 77;
    return in;
}
int comm_allgather_inplace(const l2z_comm *c, float *buf, size_t count, int gi, int n_g, bool pushed, hipStream_t st)
{
    if (c != nullptr) printf("  comm_allgather_inplace rank %d of %d buf %p count %zu gi %d of %d pushed %d stream %p\n", c->rank, c->world, P(buf), count, gi, n_g, (int)pushed, P(st));
    return 0;
}
int comm_allreduce(const l2z_comm *c, const float *part, float *out, size_t count, int gi, bool pushed, hipStream_t st)
{
    printf("  comm_allreduce rank %d of %d part %p out %p count %zu gi %d pushed %d stream %p\n", c->rank, c->world, P(part), P(out), count, gi, (int)pushed, P(st));
    return 0;
}
hipError_t launch_matvec(const MatvecArgs &a, int pro, int epi, int mb, int n_cus, hipStream_t st, int *out_grid, bool *pushed)
{
    printf("  launch_matvec pro %d epi %d max_blocks %d cus %d stream %p\n", pro, epi, mb, n_cus, P(st));
    print_mv(a);
    if (out_grid) *out_grid = 1 + (a.rows0 + a.rows1 + a.rows2) % 509;
    if (pushed) *pushed = a.push != nullptr && epi != EPI_ROPE;
    return hipSuccess;
}
hipError_t launch_q8_matvec(const Q8MatvecArgs &a, int epi, int mb, int n_cus, hipStream_t st, int *out_grid)
{
    printf("  launch_q8_matvec epi %d max_blocks %d cus %d stream %p\n", epi, mb, n_cus, P(st));
    print_mv(a.b);
    printf("    q %p %p %p s %p %p %p gs %d xq %p xs %p\n", P(a.q0), P(a.q1), P(a.q2), P(a.s0), P(a.s1), P(a.s2), a.gs, P(a.xq), P(a.xs));
    if (out_grid) *out_grid = 1 + (a.b.rows0 + a.b.rows1 + a.b.rows2) % 251;
    return hipSuccess;
}
hipError_t launch_fused_qkv_attn(const FusedQkvAttnArgs &a, int n_heads, hipStream_t st)
{
    printf("  launch_fused_qkv_attn heads %d stream %p\n", n_heads, P(st));
    printf("    w %p %p %p rms_w %p x %p q_out %p k %p v %p xb %p pos_ptr %p rope %p n %d hs %d seq_len %d kv_dim %d kv_row %d kv_head %zu\n",
           P(a.wq), P(a.wk), P(a.wv), P(a.rms_w), P(a.x), P(a.q_out), P(a.kcache), P(a.vcache), P(a.xb), P(a.pos_ptr), P(a.rope), a.n,
           a.head_size, a.seq_len, a.kv_dim, a.kv_row, a.kv_head);
    return hipSuccess;
}
hipError_t launch_attention(const AttnArgs &a, int heads, hipStream_t st, int form)
{
    printf("  launch_attention heads %d form %d stream %p\n", heads, form, P(st));
    print_attn(a);
    return hipSuccess;
}
hipError_t launch_attention_split(const AttnArgs &a, int heads, int nch, float *part, int *arrivals, hipStream_t st, bool small)
{
    printf("  launch_attention_split heads %d nch %d part %p arrivals %p small %d stream %p\n", heads, nch, P(part), P(arrivals), (int)small, P(st));
    print_attn(a);
    return hipSuccess;
}
hipError_t launch_argmax(const ArgmaxArgs &a, hipStream_t st)
{
    printf("  launch_argmax stream %p\n", P(st));
    printf("    logits %p vocab %d part %p %p %d token %p pos %p prompt %p %p out_tokens %p argmax_out %p tok_emb %p x %p dim %d emb_q8 %p %p %d "
           "advance %d epoch %p %d xchg %p %d\n", P(a.logits), a.vocab, P(a.part_val), P(a.part_idx), a.n_part, P(a.token_ptr), P(a.pos_ptr),
           P(a.prompt), P(a.n_prompt_ptr), P(a.out_tokens), P(a.argmax_out), P(a.tok_emb), P(a.x), a.dim, P(a.emb_q8.q), P(a.emb_q8.s),
           a.emb_q8.gs, a.advance, P(a.epoch_ctl), a.epoch_add, P(a.xchg), a.xchg_gi);
    return hipSuccess;
}
hipError_t launch_sample_step(const SampleStepArgs &a, hipStream_t st)
{
    printf("  launch_sample_step stream %p\n", P(st));
    printf("    logits %p vocab %d params %p coins %p seq_len %d scratch %p token %p pos %p prompt %p %p out_tokens %p tok_emb %p x %p dim %d "
           "emb_q8 %p %p %d\n", P(a.logits), a.vocab, P(a.params), P(a.coins), a.seq_len, P(a.scratch), P(a.token_ptr), P(a.pos_ptr), P(a.prompt),
           P(a.n_prompt_ptr), P(a.out_tokens), P(a.tok_emb), P(a.x), a.dim, P(a.emb_q8.q), P(a.emb_q8.s), a.emb_q8.gs);
    return hipSuccess;
}
}  // namespace l2z

// ---- the fake objects: aligned addresses nothing dereferences ----
static uintptr_t g_bump;
template <class T> static T *fake(size_t bytes) { T *p = (T *)g_bump; g_bump += (bytes + 4095) / 4096 * 4096; return p; }
static int pad_cols_(int n) { return n > 768 ? (n + 255) / 256 * 256 : (n + 3) / 4 * 4; }

static void make_state(l2z_runstate &s, const l2z_config &c, int world, int rank, bool scheme_b)
{
    s.cfg = c;
    Shard &sh = s.sh;
    const int hs = c.dim / c.n_heads;
    sh.rank = rank; sh.world = world; sh.hs = hs;
    sh.dim_loc = c.dim / world; sh.dim0 = rank * sh.dim_loc; sh.heads_loc = c.n_heads / world; sh.kvd_loc = c.n_kv_heads / world * hs;
    sh.hid_loc = c.hidden_dim / world; sh.hid0 = rank * sh.hid_loc; sh.v_loc = c.vocab_size / world; sh.v0 = rank * sh.v_loc;
    sh.scheme_b = scheme_b; sh.dimc_pad = pad_cols_(sh.dim_loc); sh.hidc_pad = pad_cols_(sh.hid_loc);
    g_bump = 0x100000000ull;
    const size_t big = (size_t)1 << 30, small = (size_t)1 << 20;
    s.x = fake<float>(small); s.xb = fake<float>(small); s.hb = fake<float>(small); s.q = fake<float>(small); s.logits = fake<float>(small);
    s.part = fake<float>(small); s.key_cache = fake<float>(big); s.value_cache = fake<float>(big); s.rope = fake<float2>(small);
    s.d_token = fake<int>(4096); s.d_pos = fake<int>(4096); s.d_prompt = fake<int>(small); s.d_n_prompt = fake<int>(4096);
    s.d_out_tokens = fake<int>(small); s.d_argmax = fake<int>(4096);
    s.d_smp_ctl = fake<float>(small); s.d_smp_scratch = fake<float>(small);
    s.d_part_val = fake<float>(small); s.d_part_idx = fake<int>(small);
    s.d_attn_part = fake<float>(small); s.d_attn_cnt = fake<int>(small);
    s.attn_nch = 4; s.max_blocks = 8; s.use_graphs = false;
    s.n_gathers = (scheme_b ? 2 : 4) * c.n_layers + 1;
}

static void make_weights(l2z_weights &w, const l2z_config &c, const Shard &sh, int gs)
{
    w.cfg = c; w.sh = sh; w.shared = 0; w.uid = 1;
    g_bump = 0x4000000000ull;
    const size_t big = (size_t)1 << 32;
    w.rms_att = fake<float>(big); w.rms_ffn = fake<float>(big); w.rms_final = fake<float>(big);
    if (gs == 0) {
        const float **ws[] = {&w.tok_emb, &w.wq, &w.wk, &w.wv, &w.wo, &w.w1, &w.w2, &w.wcls};
        for (const float **q : ws) *q = fake<float>(big);
        w.w3 = w.w1 + c.dim;
        return;
    }
    w.q8_gs = gs;
    l2z_weights::Q8Mat *ms[] = {&w.q_emb, &w.q_wq, &w.q_wk, &w.q_wv, &w.q_wo, &w.q_w13, &w.q_w2, &w.q_cls};
    for (auto *m : ms) { m->q = fake<int8_t>(big); m->s = fake<float>(big); }
}

// packed slots of every kind: form 1 all at 29 bits, 2 ffn13 and cls at 28, 3 at 29 with slot 1 (Wk) of the last layer's q|k|v missing
static void pack_weights(l2z_weights &w, int form)
{
    const l2z_config &c = w.cfg;
    g_bump = 0x8000000000ull;
    const int kinds[] = {KIND_QKV, KIND_WO, KIND_FFN13, KIND_FFN2, KIND_CLS};
    for (int k : kinds) {
        l2z_weights::PkKind &pk = w.pk[k];
        pk.blob = fake<uint32_t>((size_t)1 << 32);
        pk.per_layer = k == KIND_QKV ? 3 : 1;
        const int n = k == KIND_CLS ? 1 : c.n_layers * pk.per_layer;
        for (int i = 0; i < n; i++) {
            l2z_weights::PkMat m;
            m.p = fake<uint32_t>((size_t)1 << 28);
            m.e = 100 + 7 * k + i;
            if (form == 2 && (k == KIND_FFN13 || k == KIND_CLS)) m.rec = fake<uint32_t>((size_t)1 << 24);
            if (form == 3 && k == KIND_QKV && i == n - 2) m.p = nullptr;
            pk.slots.push_back(m);
            pk.packed += m.p != nullptr;
        }
    }
}

static const char *kStep[] = {"none", "greedy", "sample"};

static void one(l2z_runstate &s, const l2z_weights &w, int step, bool prof_on, int only_stage, int variant, int only_kind)
{
    printf("- step %s prof %d only_stage %d variant %d only_kind %d\n", kStep[step], (int)prof_on, only_stage, variant, only_kind);
    Prof prof;
    g_ev = 0x10;
    s.n_part = 0; s.n_part_step = -1; s.n_part_fwd = -1; s.logits_partial = false; s.tl_attn_seq = 5;
    const int rc = enqueue_forward(&s, &w, (StepKind)step, prof_on ? &prof : nullptr, only_stage, variant, only_kind);
    printf("  -> %d n_part %d step %d fwd %d logits_partial %d tl_attn_seq %d kinds", rc, s.n_part, s.n_part_step, s.n_part_fwd,
           (int)s.logits_partial, s.tl_attn_seq);
    for (int k : prof.kind) printf(" %d", k);
    printf("\n");
}

static void sweep(l2z_runstate &s, const l2z_weights &w)
{
    for (int step = 0; step <= 2; step++)
        for (int variant = 0; variant < ATTN_VARIANTS; variant++)
            for (int only_kind = -1; only_kind < KIND_GATHER; only_kind++)
                for (int prof_on = 0; prof_on <= (only_kind < 0 ? 1 : 0); prof_on++) one(s, w, step, prof_on != 0, -1, variant, only_kind);
}

static void run_shape(const char *name, const l2z_config &c, bool fused)
{
    // ---- unsharded ----
    for (int form = 0; form <= 3; form++) {
        static const int masks[] = {-1, 0, 1 << KIND_QKV, 1 << KIND_WO, 1 << KIND_FFN13, 1 << KIND_FFN2, 1 << KIND_CLS};
        for (int mask : masks) {
            if (form == 0 && mask != -1) continue;
            for (int packed_w = 1; packed_w >= (mask == -1 && form == 1 ? 0 : 1); packed_w--) {
                l2z_runstate s = {};
                make_state(s, c, 1, 0, false);
                s.fused_qkv_attn = fused; s.packed_kinds = mask; s.packed_w = packed_w != 0;
                l2z_weights w = {};
                make_weights(w, c, s.sh, 0);
                if (form) pack_weights(w, form);
                printf("== %s f32 packed form %d kinds mask %d packed_w %d\n", name, form, mask, packed_w);
                sweep(s, w);
            }
        }
    }
    for (int gs : {32, 64}) {
        if (c.dim % gs || c.hidden_dim % gs) continue;
        l2z_runstate s = {};
        make_state(s, c, 1, 0, false);
        s.fused_qkv_attn = fused;
        l2z_weights w = {};
        make_weights(w, c, s.sh, gs);
        printf("== %s q8 gs %d\n", name, gs);
        sweep(s, w);
        printf("== %s q8 gs %d refusals\n", name, gs);
        one(s, w, 1, false, 0, ATTN_HEAD, -1);
        one(s, w, 0, false, 3, ATTN_HEAD, -1);
        s.sh.world = 2;
        one(s, w, 1, false, -1, ATTN_HEAD, -1);
        one(s, w, 1, false, 2, ATTN_HEAD, -1);
    }
    // ---- ranks 0 and 1 of 2 ----
    if (c.n_kv_heads % 2) return;
    for (int sb = 0; sb <= 1; sb++)
        for (int rank = 0; rank <= 1; rank++) {
            l2z_comm comm = {};
            comm.rank = rank; comm.world = 2;
            comm.arena = (char *)0x7000000000ull; comm.slot_floats = 1 << 20; comm.d_ctl = (int *)0x7100000000ull; comm.h_err = (int *)0x7200000000ull;
            // emulated ranks: stage by stage (l2z_emu_transformer), and kind by kind (l2z_time_kind)
            {
                l2z_runstate s = {};
                make_state(s, c, 2, rank, sb != 0);
                s.comm = &comm;
                l2z_weights w = {};
                make_weights(w, c, s.sh, 0);
                printf("== %s rank %d of 2 scheme_b %d emulated\n", name, rank, sb);
                const int n_stages = (sb ? 2 : 4) * c.n_layers + 1;
                for (int stage = 0; stage <= n_stages; stage++)
                    for (int step = 0; step <= 1; step++) one(s, w, step, false, stage, stage % ATTN_VARIANTS, -1);
                for (int only_kind = 0; only_kind < KIND_GATHER; only_kind++) one(s, w, 1, false, -1, ATTN_HEAD, only_kind);
                one(s, w, 1, true, -1, ATTN_SPLIT, -1);
            }
            // the peer-write transport: gather launches, consumer-side words, the candidate exchange, a solo rank
            for (int consume = 0; consume <= 1; consume++)
                for (int xchg = 0; xchg <= 1; xchg++)
                    for (int solo = 0; solo <= 1; solo++) {
                        l2z_runstate s = {};
                        make_state(s, c, 2, rank, sb != 0);
                        comm.p2p = true; comm.solo = solo != 0;
                        s.comm = &comm;
                        s.d_push = (P2pArgs *)0x7300000000ull; s.ll_consume = consume != 0; s.xchg_steps = xchg != 0;
                        l2z_weights w = {};
                        make_weights(w, c, s.sh, 0);
                        pack_weights(w, 1);   // (a shard never streams a packed copy, whatever the object holds)
                        printf("== %s rank %d of 2 scheme_b %d p2p consume %d xchg %d solo %d\n", name, rank, sb, consume, xchg, solo);
                        for (int step = 0; step <= 1; step++)
                            for (int prof_on = 0; prof_on <= 1; prof_on++) one(s, w, step, prof_on != 0, -1, step ? ATTN_SPLIT_S : ATTN_SHORT, -1);
                        if (solo) for (int only_kind = 0; only_kind < KIND_GATHER; only_kind++) one(s, w, 1, false, -1, ATTN_HEAD, only_kind);
                    }
            comm.p2p = false; comm.solo = false;
        }
}

int main()
{
    const l2z_config gqa = {512, 1408, 2, 8, 4, 1024, 64}, mha = {288, 768, 3, 6, 6, 1024, 32}, b7 = {4096, 11008, 2, 32, 32, 32000, 2048};
    run_shape("gqa", gqa, false);
    run_shape("mha", mha, true);
    run_shape("7B", b7, false);
    return 0;
}
