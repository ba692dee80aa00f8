// owned_check.cpp -- the owner type and the grow rule of llama2.zig_amd/csrc/owned.h on the host (tests/test_owned_host.py
// builds it with the address and undefined-behaviour sanitizers and runs it).  The two raw functions are this file's, over
// malloc: they keep the set of live pointers, abort on a free of a pointer that is not in it, and fail the N-th allocation
// on request.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "owned.h"

using namespace l2z;

namespace {
std::set<void *> g_live;
int g_allocs = 0, g_frees = 0, g_fail_at = 0;   // g_fail_at: the allocation (1-based, counted from its setting) that fails
int g_drains = 0;
constexpr int kOom = -4;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

int drain()
{
    g_drains++;
    return 0;
}
}  // namespace

int l2z::raw_alloc(Mem, void **p, size_t bytes, const char *)
{
    *p = nullptr;
    if (g_fail_at > 0 && --g_fail_at == 0) return kOom;
    *p = malloc(bytes);
    REQUIRE(*p != nullptr);
    g_live.insert(*p);
    g_allocs++;
    return 0;
}

void l2z::raw_free(Mem, void *p)
{
    if (g_live.erase(p) != 1) {
        printf("FAILED: free of %p, which is not live\n", p);
        abort();
    }
    free(p);
    g_frees++;
}

namespace {

// a group as the runstate holds them: K = 4 members of two kinds, one of them without a size at this shape
struct Group {
    Owned<float> a;
    Owned<int> none;   // zero-sized: stays null
    Pinned<float> b;
    Owned<void> c;
    int cap = 0, key = 0;
    int grow_to(int need, int want_key, bool *remade = nullptr)
    {
        const size_t P = (size_t)round_cap(need, 512);
        return grow("check", &cap, need, 512, &key, want_key, drain, {{a, P * 4}, {none, 0}, {b, P * 8}, {c, P + 16}}, remade);
    }
    bool empty() const { return a == nullptr && none == nullptr && b == nullptr && c == nullptr && cap == 0 && key == 0; }
};

void move_frees_once()
{
    const int frees = g_frees;
    {
        Owned<float> x;
        REQUIRE(x.get() == nullptr && x.make(64, "x") == 0 && x != nullptr);
        float *was = x;
        REQUIRE(x.make(128, "x") == 0 && x == was);   // make if absent: it is there
        Owned<float> y(std::move(x));
        REQUIRE(x.get() == nullptr && y == was && g_live.size() == 1);
        Owned<float> z;
        REQUIRE(z.make(32, "z") == 0);
        z = std::move(y);   // z's own goes, y's comes
        REQUIRE(y.get() == nullptr && z == was && g_live.size() == 1 && g_frees == frees + 1);
    }
    REQUIRE(g_live.empty() && g_frees == frees + 2);
    printf("ok: move leaves the source null and frees once\n");
}

void reset_twice()
{
    Owned<int> x;
    x.reset();
    REQUIRE(x.make(16, "x") == 0);
    const int frees = g_frees;
    x.reset();
    x.reset();
    REQUIRE(x.get() == nullptr && g_frees == frees + 1 && g_live.empty());
    printf("ok: reset twice is harmless\n");
}

void grow_cases()
{
    Group g;
    bool remade = false;
    REQUIRE(g.grow_to(1, 32, &remade) == 0 && remade && g.cap == 512 && g.key == 32 && g.none == nullptr && g_live.size() == 3);
    void *a = g.a.get();
    int allocs = g_allocs, frees = g_frees, drains = g_drains;
    REQUIRE(g.grow_to(512, 32, &remade) == 0 && !remade && g.grow_to(7, 32) == 0);
    REQUIRE(g_allocs == allocs && g_frees == frees && g_drains == drains && g.a.get() == a && g.cap == 512);
    printf("ok: grow at the same capacity and key allocates nothing\n");

    REQUIRE(g.grow_to(513, 32, &remade) == 0 && remade);
    REQUIRE(g_drains == drains + 1 && g_frees == frees + 3 && g_allocs == allocs + 3 && g.cap == 1024 && g.key == 32 && g_live.size() == 3);
    printf("ok: grow to a larger need drains, frees each old member once and records the rounded capacity\n");

    allocs = g_allocs; frees = g_frees;
    REQUIRE(g.grow_to(1024, 64, &remade) == 0 && remade);
    REQUIRE(g_frees == frees + 3 && g_allocs == allocs + 3 && g.cap == 1024 && g.key == 64 && g_live.size() == 3);
    printf("ok: a changed key at an equal capacity remakes the group\n");
}

void every_failure_empties_the_group()
{
    const int K = 4, needs[] = {1, 512, 513};
    for (int need : needs)
        for (int held = 0; held < 2; held++)        // from an empty group, and from one that holds a smaller capacity's
            for (int n = 1; n <= K - 1; n++) {      // (the zero-sized member allocates nothing: K - 1 allocations)
                Group g;
                if (held) REQUIRE(g.grow_to(need, 32) == 0 && g.grow_to(need, 32) == 0);
                g_fail_at = n;
                REQUIRE(g.grow_to(held ? need + 512 : need, 32) == kOom);
                REQUIRE(g_fail_at == 0 && g.empty() && g_live.empty());
                bool remade = false;
                REQUIRE(g.grow_to(need, 32, &remade) == 0 && remade && g.cap == round_cap(need, 512) && g.key == 32 && g_live.size() == 3);
            }
    REQUIRE(g_live.empty());
    printf("ok: a failed allocation leaves the group empty, and the next grow succeeds\n");
}

void half_built_struct_frees_itself()
{
    {
        Group g;   // members made one by one, as a scratch struct is built in a local owner before it is installed
        REQUIRE(g.a.make(64, "a") == 0);
        g_fail_at = 1;
        REQUIRE(g.b.make(64, "b") == kOom && g.b == nullptr);
        REQUIRE(g_live.size() == 1);
    }
    REQUIRE(g_live.empty());
    printf("ok: destroying an owner struct with a half-built group leaves the live set empty\n");
}

}  // namespace

int main()
{
    move_frees_once();
    reset_twice();
    grow_cases();
    every_failure_empties_the_group();
    half_built_struct_frees_itself();
    REQUIRE(g_live.empty() && g_allocs == g_frees);
    return 0;
}
