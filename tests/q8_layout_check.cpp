// q8_layout_check.cpp -- llama2.zig_amd/csrc/q8_layout.h on its own: a stand-alone program (tests/test_q8_layout_host.py
// builds it with -fsanitize=address,undefined and runs it).  Every case prints "ok: <case>" or the program exits non-zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "q8_layout.h"

using namespace l2z::q8;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static const Dims kStories15M = {288, 768, 6, 6, 6, 32000, 256};
static const Dims kStories42M = {512, 1376, 8, 8, 8, 32000, 1024};
static const Dims kStories110M = {768, 2048, 12, 12, 12, 32000, 1024};
static const Dims kLlama7B = {4096, 11008, 32, 32, 32, 32000, 2048};
static const Dims kTiny = {64, 192, 2, 4, 2, 512, 32};

// the total by the format's own words: three norm tensors, then values + one f32 scale per group of every matrix
static uint64_t total_by_hand(const Dims &c, bool shared, int gs)
{
    const uint64_t dim = c.dim, hid = c.hidden_dim, L = c.n_layers, V = c.vocab_size, kvd = dim / c.n_heads * c.n_kv_heads;
    uint64_t values = V * dim + L * (dim * dim + 2 * kvd * dim + dim * dim + 3 * hid * dim);
    if (!shared) values += V * dim;
    return 4 * (2 * L * dim + dim) + values + values / gs * 4;
}

static void totals()
{
    Layout lay;
    const struct { const Dims *c; bool shared; int gs; } cases[] = {
        {&kStories15M, true, 32}, {&kStories42M, true, 32}, {&kStories110M, true, 32}, {&kStories110M, true, 64},
        {&kLlama7B, false, 32},   {&kLlama7B, false, 64},   {&kTiny, true, 32},        {&kTiny, false, 64}};
    for (const auto &k : cases) {
        CHECK(layout(*k.c, k.shared, k.gs, &lay) == LAYOUT_OK);
        CHECK(lay.total == total_by_hand(*k.c, k.shared, k.gs));
        CHECK(lay.gs == k.gs);
    }
    CHECK(layout(kLlama7B, false, 64, &lay) == LAYOUT_OK);
    CHECK(lay.total > (uint64_t)1 << 32);   // past 32 bits: the offsets are 64-bit
    CHECK(lay.t[T_CLS].present && lay.t[T_CLS].s_off + lay.t[T_CLS].values() / 64 * 4 == lay.total);
    std::printf("ok: totals of the named shapes\n");
}

static void order_and_cover()
{
    // every byte of the body belongs to exactly one piece, the pieces come in the file's order
    for (int shared = 0; shared < 2; shared++) {
        for (int gs : {32, 64}) {
            Layout lay;
            CHECK(layout(kTiny, shared != 0, gs, &lay) == LAYOUT_OK);
            std::vector<unsigned char> body(lay.total, 0);
            const auto mark = [&](uint64_t off, uint64_t n) {
                for (uint64_t i = 0; i < n; i++) body.at(off + i)++;
            };
            const uint64_t L = kTiny.n_layers, dim = kTiny.dim;
            CHECK(lay.rms_att_off == 0 && lay.rms_ffn_off == 4 * L * dim && lay.rms_final_off == 8 * L * dim);
            mark(lay.rms_att_off, 4 * L * dim);
            mark(lay.rms_ffn_off, 4 * L * dim);
            mark(lay.rms_final_off, 4 * dim);
            uint64_t at = lay.rms_final_off + 4 * dim;
            for (int t = 0; t < T_COUNT; t++) {
                const Mat &m = lay.t[t];
                if (t == T_CLS) CHECK(m.present == (shared == 0));
                if (!m.present) continue;
                CHECK(m.q_off == at && m.s_off == at + m.values());
                CHECK(m.values() % gs == 0 && m.s_off % 4 == 0);
                mark(m.q_off, m.values());
                mark(m.s_off, m.values() / gs * 4);
                at = m.s_off + m.values() / gs * 4;
            }
            CHECK(at == lay.total);
            for (unsigned char b : body) CHECK(b == 1);
            CHECK(lay.t[T_WK].rows == 32 && lay.t[T_WK].cols == 64 && lay.t[T_W2].cols == 192 && lay.t[T_W1].rows == 192);
            CHECK(lay.t[T_EMB].layers == 1 && lay.t[T_WQ].layers == L);
        }
    }
    std::printf("ok: the pieces cover the body once, in the file's order\n");
}

static void refusals()
{
    Layout lay;
    std::memset(&lay, 0x5a, sizeof lay);
    for (int gs : {0, -32, 1, 16, 48, 128, 256}) CHECK(layout(kTiny, true, gs, &lay) == BAD_GROUP_SIZE);
    CHECK(layout(kStories15M, true, 64, &lay) == NOT_DIVISIBLE);      // dim 288
    CHECK(layout(kStories42M, true, 64, &lay) == NOT_DIVISIBLE);      // hidden_dim 1376
    Dims d = kTiny;
    d.dim = 0;
    CHECK(layout(d, true, 32, &lay) == BAD_DIMS);
    d = kTiny; d.n_layers = -1;
    CHECK(layout(d, true, 32, &lay) == BAD_DIMS);
    d = kTiny; d.n_heads = 3;
    CHECK(layout(d, true, 32, &lay) == BAD_DIMS);
    d = kTiny; d.n_kv_heads = 3;
    CHECK(layout(d, true, 32, &lay) == BAD_DIMS);
    d = kTiny; d.vocab_size = 0;
    CHECK(layout(d, true, 32, &lay) == BAD_DIMS);
    CHECK(layout(kTiny, true, 32, &lay) == LAYOUT_OK);
    const uint64_t total = lay.total;
    CHECK(layout_checked(kTiny, true, 32, total, &lay) == LAYOUT_OK);
    CHECK(layout_checked(kTiny, true, 32, total + 100, &lay) == LAYOUT_OK);
    CHECK(layout_checked(kTiny, true, 32, total - 1, &lay) == BODY_TOO_SHORT);
    CHECK(layout_checked(kTiny, true, 32, 0, &lay) == BODY_TOO_SHORT);
    CHECK(layout_checked(kTiny, false, 32, total, &lay) == BODY_TOO_SHORT);   // a shared file read as unshared
    CHECK(layout_checked(kTiny, true, 16, total, &lay) == BAD_GROUP_SIZE);
    for (int st = LAYOUT_OK; st <= BODY_TOO_SHORT; st++) CHECK(status_text(st) != nullptr && status_text(st)[0] != 0);
    std::printf("ok: refusals\n");
}

static void names()
{
    for (int t = 0; t < T_COUNT; t++) CHECK(tensor_by_name(kTensorNames[t]) == t);
    CHECK(tensor_by_name("w") == -1 && tensor_by_name("wqq") == -1 && tensor_by_name("") == -1 && tensor_by_name(nullptr) == -1);
    CHECK(tensor_by_name("rms_att_weight") == -1);
    std::printf("ok: tensor names\n");
}

int main()
{
    totals();
    order_and_cover();
    refusals();
    names();
    return 0;
}
