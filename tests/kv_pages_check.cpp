// kv_pages_check.cpp -- a stand-alone program over llama2.zig_amd/csrc/kv_pages.h alone (no HIP, nothing of the library):
// the paged KV cache's host bookkeeping, case by case.  tests/test_kv_pages_host.py builds it with
// -fsanitize=address,undefined and runs it; it prints one line per case and exits 0 when every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kv_pages.h"

using namespace l2z;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            g_failed++;                                                  \
        }                                                                \
    } while (0)

static void missing_for_a_range()
{
    KvPages pool(8);
    KvSeq s;
    s.init(320);   // 5 pages
    CHECK(s.pages.size() == 5 && s.n_attached() == 0);
    CHECK(pool.missing(s, 0, 0) == 0);        // an empty range
    CHECK(pool.missing(s, 0, 1) == 1);
    CHECK(pool.missing(s, 63, 64) == 1);      // position 63 alone: page 0
    CHECK(pool.missing(s, 63, 65) == 2);      // 63 and 64: pages 0 and 1
    CHECK(pool.missing(s, 64, 128) == 1);     // exactly page 1
    CHECK(pool.missing(s, 0, 320) == 5);
    CHECK(pool.attach(s, 64, 65));
    CHECK(pool.missing(s, 0, 320) == 4 && pool.missing(s, 64, 128) == 0 && pool.missing(s, 127, 129) == 1);
    CHECK(s.pages[0] == -1 && s.pages[1] == 0 && pool.refs(0) == 1);   // a fresh pool hands out 0, 1, 2, ...
}

static void attach_then_release_restores_the_free_count()
{
    KvPages pool(6);
    KvSeq a, b;
    a.init(256);
    b.init(256);
    CHECK(pool.n_free() == 6 && pool.n_pages() == 6);
    CHECK(pool.attach(a, 0, 130));            // pages 0, 1, 2
    CHECK(pool.attach(b, 0, 64));             // page 0
    CHECK(pool.attach(a, 100, 130));          // nothing new
    CHECK(pool.n_free() == 2 && a.n_attached() == 3 && b.n_attached() == 1);
    CHECK(pool.release(a, 65) == 1);          // trim: page 2 lies wholly at or above 65, page 1 does not
    CHECK(pool.n_free() == 3 && a.pages[2] == -1 && a.pages[1] >= 0);
    CHECK(pool.release(a, 64) == 1);          // page 1 starts at 64
    CHECK(pool.release(a) == 1 && pool.release(a) == 0);
    CHECK(pool.release(b) == 1);
    CHECK(pool.n_free() == 6);
    for (int p = 0; p < 6; p++) CHECK(pool.refs(p) == 0);
    // the page given back last goes out first: the lists of later sequences are not ascending
    KvSeq c;
    c.init(256);
    CHECK(pool.attach(c, 0, 128));
    CHECK(c.pages[0] == 3 && c.pages[1] == 0);   // b's page came back last, then a's page 0
    std::vector<int> seen(6, 0);
    KvSeq d;
    d.init(256);
    CHECK(pool.attach(d, 0, 256));
    for (int32_t id : c.pages) if (id >= 0) seen[(size_t)id]++;
    for (int32_t id : d.pages) if (id >= 0) seen[(size_t)id]++;
    for (int p = 0; p < 6; p++) CHECK(seen[(size_t)p] == 1);   // every page handed out exactly once
    CHECK(pool.n_free() == 0);
}

static void share_and_release_in_either_order()
{
    for (int order = 0; order < 2; order++) {
        KvPages pool(8);
        KvSeq src, dst;
        src.init(320);
        dst.init(320);
        CHECK(pool.attach(src, 0, 200));      // pages 0 .. 3
        pool.share(dst, src, 130 / kKvPage);  // a fork at 130: two whole pages
        CHECK(pool.attach(dst, 128, 130));    // and a private third
        CHECK(pool.n_free() == 3);
        CHECK(dst.pages[0] == src.pages[0] && dst.pages[1] == src.pages[1] && dst.pages[2] != src.pages[2]);
        CHECK(pool.refs(src.pages[0]) == 2 && pool.refs(src.pages[1]) == 2 && pool.refs(src.pages[2]) == 1 &&
              pool.refs(dst.pages[2]) == 1);
        KvSeq &first = order == 0 ? src : dst, &second = order == 0 ? dst : src;
        const int32_t shared0 = src.pages[0];
        pool.release(first);
        CHECK(pool.refs(shared0) == 1);       // still held by the other one
        CHECK(pool.n_free() == (order == 0 ? 5 : 4));
        CHECK(second.pages[0] == shared0);
        pool.release(second);
        CHECK(pool.n_free() == 8 && pool.refs(shared0) == 0);
    }
}

static void shared_page_write_refusal()
{
    KvPages pool(8);
    KvSeq src, dst;
    src.init(320);
    dst.init(320);
    CHECK(pool.attach(src, 0, 200));
    CHECK(!pool.writes_shared(src, 0, 200));
    pool.share(dst, src, 2);
    CHECK(pool.attach(dst, 128, 130));
    CHECK(pool.writes_shared(dst, 100, 101));     // a rewind below the fork point
    CHECK(pool.writes_shared(src, 127, 128));     // the source too: the page is no longer its own
    CHECK(pool.writes_shared(dst, 127, 129));     // a range that only starts in a shared page
    CHECK(!pool.writes_shared(dst, 128, 192));    // its private page
    CHECK(!pool.writes_shared(src, 128, 320));    // private pages and pages not attached yet
    CHECK(!pool.writes_shared(dst, 100, 100));    // an empty range
    pool.release(src);
    CHECK(!pool.writes_shared(dst, 100, 101));    // the last holder may write
}

static void exhaustion_attaches_nothing()
{
    KvPages pool(3);
    KvSeq a, b;
    a.init(512);
    b.init(512);
    CHECK(pool.attach(a, 0, 100));                // 2 pages
    const std::vector<int32_t> before = b.pages;
    CHECK(pool.missing(b, 0, 65) == 2 && pool.n_free() == 1);
    CHECK(!pool.attach(b, 0, 65));                // needs 2, 1 free
    CHECK(b.pages == before && b.n_attached() == 0 && pool.n_free() == 1);
    CHECK(!pool.attach(a, 100, 300));             // a's own growth too: pages 2, 3, 4
    CHECK(a.n_attached() == 2 && pool.n_free() == 1);
    CHECK(pool.attach(b, 0, 64));                 // what fits still goes
    CHECK(pool.n_free() == 0 && !pool.attach(b, 64, 65) && b.n_attached() == 1);
    pool.release(a, 64);
    CHECK(pool.n_free() == 1 && pool.attach(b, 64, 65));
}

static void seq_len_not_a_multiple_of_the_page()
{
    CHECK(kv_pages_for(0) == 0 && kv_pages_for(1) == 1 && kv_pages_for(64) == 1 && kv_pages_for(65) == 2);
    KvPages pool(4);
    KvSeq s;
    s.init(160);                                  // 2 whole pages and one of 32 rows
    CHECK(s.pages.size() == 3);
    CHECK(pool.missing(s, 159, 160) == 1 && pool.missing(s, 0, 160) == 3);
    CHECK(pool.attach(s, 0, 160));
    CHECK(s.n_attached() == 3 && pool.n_free() == 1);
    CHECK(pool.release(s, 129) == 0);             // the last page holds 128: not wholly at or above 129
    CHECK(pool.release(s, 128) == 1 && pool.n_free() == 2);
    KvSeq one;
    one.init(1);
    CHECK(one.pages.size() == 1 && pool.attach(one, 0, 1) && pool.release(one, 1) == 0 && pool.release(one, 0) == 1);
}

int main()
{
    struct { const char *name; void (*fn)(); } cases[] = {
        {"pages missing for a position range", missing_for_a_range},
        {"attach, then release restores the free count", attach_then_release_restores_the_free_count},
        {"share and release by reference count in either order", share_and_release_in_either_order},
        {"the shared-page write refusal", shared_page_write_refusal},
        {"exhaustion is reported with nothing attached", exhaustion_attaches_nothing},
        {"seq_len not a multiple of 64", seq_len_not_a_multiple_of_the_page},
    };
    for (const auto &c : cases) {
        const int before = g_failed;
        c.fn();
        printf("%s: %s\n", g_failed == before ? "ok" : "FAILED", c.name);
    }
    return g_failed == 0 ? 0 : 1;
}
