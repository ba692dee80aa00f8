// kv_pool.cpp -- the device side of the paged KV cache (include/llama2_hip_test.h l2z_kvpool; the
// bookkeeping itself: kv_pages.h): the pool's two arrays, a paged runstate's page table and its copy on the device, what the
// wide family's entry points do before they enqueue (kv_check_kind, kv_attach, kv_upload), and the strided copies behind
// l2z_runstate_fork and l2z_runstate_read.  There is no device-side allocation: every page a pass touches was attached on
// the host before the pass was enqueued.
#include <algorithm>
#include <cstring>

#include "batch_host.h"

static_assert(l2z::kKvPage == L2Z_KV_PAGE, "include/llama2_hip_test.h L2Z_KV_PAGE");
static_assert(l2z::kKvPage == l2z::kVerifySeg, "a page is a segment of the verify / wide attention");

namespace l2z {

int kv_check_kind(const char *fn, int n, l2z_runstate *const *states)
{
    const l2z_kvpool *pool = states[0]->pool;
    for (int i = 1; i < n; i++) {
        L2Z_CHECK((states[i]->pool != nullptr) == (pool != nullptr), L2Z_ERR_INVALID,
                  "%s: states[%d] is %s, states[0] is not (the runstates of a call are all contiguous or all paged)", fn, i,
                  states[i]->pool ? "paged" : "contiguous");
        L2Z_CHECK(states[i]->pool == pool, L2Z_ERR_INVALID, "%s: states[%d] draws its pages from another pool than states[0]", fn, i);
    }
    return L2Z_OK;
}

int kv_attach(const char *fn, int n, l2z_runstate *const *states, const int32_t *pos0, const int32_t *counts, int count)
{
    l2z_kvpool *pool = states[0]->pool;
    if (pool == nullptr) return L2Z_OK;
    int need = 0;
    for (int j = 0; j < n; j++) {
        const int a = pos0[j], b = a + (counts ? counts[j] : count);
        L2Z_CHECK(!pool->alloc.writes_shared(states[j]->pg, a, b), L2Z_ERR_STATE,
                  "%s: states[%d] would write positions %d .. %d into a page it shares with another runstate (a fork's "
                  "whole pages are shared; copy-on-write is not implemented)", fn, j, a, b - 1);
        // (the pass reads every row below a through the page table: a page it would not find is refused here, never read)
        // (rows below a in a's own page are the page's, zero or stale, as a contiguous cache's unwritten rows are)
        L2Z_CHECK(pool->alloc.missing(states[j]->pg, 0, a / kKvPage * kKvPage) == 0, L2Z_ERR_STATE,
                  "%s: states[%d] holds no page for some position below %d (given back by a trim, or never written)", fn, j,
                  a / kKvPage * kKvPage);
        need += pool->alloc.missing(states[j]->pg, a, b);
    }
    L2Z_CHECK(need <= pool->alloc.n_free(), L2Z_ERR_OOM, "%s: the call needs %d more KV pages, the pool has %d free of %d", fn,
              need, pool->alloc.n_free(), pool->alloc.n_pages());
    if (need == 0) return L2Z_OK;
    for (int j = 0; j < n; j++) {
        l2z_runstate *s = states[j];
        const int a = pos0[j], b = a + (counts ? counts[j] : count);
        if (pool->alloc.missing(s->pg, a, b) == 0) continue;
        (void)pool->alloc.attach(s->pg, a, b);   // (cannot fall short: counted above)
        s->pages_dirty = true;
    }
    return L2Z_OK;
}

int kv_upload(int n, l2z_runstate *const *states, hipStream_t st)
{
    for (int j = 0; j < n; j++) {
        l2z_runstate *s = states[j];
        if (s->pool == nullptr || !s->pages_dirty) continue;
        // (the pinned twin may be rewritten while an earlier copy of it is still queued: between two releases a table only
        // gains entries, and a release drains the stream every such copy is ordered before)
        memcpy(s->h_pages, s->pg.pages.data(), s->pg.pages.size() * 4);
        L2Z_HIP(hipMemcpyAsync(s->d_pages, s->h_pages, s->pg.pages.size() * 4, hipMemcpyHostToDevice, st));
        s->pages_dirty = false;
    }
    return L2Z_OK;
}

void kv_seq_base(const l2z_runstate *s, RaggedSeq *q)
{
    q->kc = s->pool ? s->pool->k : s->key_cache;
    q->vc = s->pool ? s->pool->v : s->value_cache;
    q->pages = s->pool ? s->d_pages : nullptr;
}

int kv_release(l2z_runstate *s, int n_pos)
{
    if (s->pool == nullptr) return L2Z_OK;
    bool any = false;
    for (size_t p = (size_t)kv_pages_for(n_pos); p < s->pg.pages.size(); p++) any = any || s->pg.pages[p] >= 0;
    if (!any) return L2Z_OK;
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_HIP(hipStreamSynchronize(s->stream));
    s->pool->alloc.release(s->pg, n_pos);
    s->pages_dirty = true;
    return L2Z_OK;
}

namespace {

// where rows lo .. of page-or-cache `p` of s start in its key (key) or value array, and the floats between two (layer, kv
// head) runs there
const float *kv_rows(const l2z_runstate *s, bool key, int lo, size_t hs, size_t *pitch)
{
    if (s->pool != nullptr) {
        *pitch = (size_t)kKvPage * hs;
        return (key ? s->pool->k : s->pool->v) + (size_t)s->pg.pages[(size_t)(lo / kKvPage)] * s->pool->page_floats +
               (size_t)(lo % kKvPage) * hs;
    }
    *pitch = (size_t)s->cfg.seq_len * hs;
    return (key ? s->key_cache : s->value_cache) + (size_t)lo * hs;
}

}  // namespace

int kv_copy_rows(l2z_runstate *dst, const l2z_runstate *src, int r0, int n_pos)
{
    const l2z_config &c = src->cfg;
    const size_t hs = (size_t)c.dim / c.n_heads, runs = (size_t)c.n_layers * c.n_kv_heads;
    // one strided copy per page's worth of rows and array (contiguous on both sides: one in all)
    const int step = dst->pool != nullptr || src->pool != nullptr ? kKvPage : c.seq_len;
    for (int lo = r0; lo < n_pos;) {
        const int hi = std::min(n_pos, (lo / step + 1) * step);
        for (int key = 0; key < 2; key++) {
            size_t sp = 0, dp = 0;
            const float *from = kv_rows(src, key != 0, lo, hs, &sp);
            float *to = (float *)kv_rows(dst, key != 0, lo, hs, &dp);
            L2Z_HIP(hipMemcpy2DAsync(to, dp * 4, from, sp * 4, (size_t)(hi - lo) * hs * 4, runs, hipMemcpyDeviceToDevice,
                                     dst->stream));
        }
        lo = hi;
    }
    return L2Z_OK;
}

void kv_runstate_free(l2z_runstate *s)
{
    if (s->pool == nullptr) return;
    s->pool->alloc.release(s->pg);   // (l2z_runstate_free has drained the stream)
    s->pool->live--;
    if (s->d_pages) (void)hipFree(s->d_pages);
    if (s->h_pages) (void)hipHostFree(s->h_pages);
    s->d_pages = s->h_pages = nullptr;
    s->pool = nullptr;
}

}  // namespace l2z

using namespace l2z;

extern "C" int l2z_kvpool_init(const l2z_config *config, int n_pages, l2z_kvpool **out)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(config != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_kvpool_init: null argument");
    L2Z_CHECK(n_pages >= 1, L2Z_ERR_INVALID, "l2z_kvpool_init: n_pages = %d (at least 1)", n_pages);
    const l2z_config &c = *config;
    L2Z_CHECK(c.dim > 0 && c.n_heads > 0 && c.n_kv_heads > 0 && c.n_layers > 0 && c.seq_len > 0 && c.dim % c.n_heads == 0 &&
                  c.n_heads % c.n_kv_heads == 0 && (c.dim / c.n_heads) % 4 == 0,
              L2Z_ERR_INVALID, "l2z_kvpool_init: the config's heads do not take the wide family (head_size a multiple of 4)");
    const int dev = current_device_for(nullptr);
    L2Z_TRY(ensure_device(dev));
    l2z_kvpool *p = new l2z_kvpool();
    p->cfg = c;
    p->device = dev;
    p->page_floats = (size_t)c.n_layers * c.n_kv_heads * kKvPage * (size_t)(c.dim / c.n_heads);
    p->alloc.reset(n_pages);
    const size_t bytes = (size_t)n_pages * p->page_floats * 4;
    hipError_t e = hipMalloc((void **)&p->k, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&p->v, bytes);
    // zero once: a row no pass has written yet is never a NaN bit pattern (recycled pages are NOT cleared)
    if (e == hipSuccess) e = hipMemset(p->k, 0, bytes);
    if (e == hipSuccess) e = hipMemset(p->v, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("l2z_kvpool_init: %d pages of %zu bytes: %s", n_pages, 2 * p->page_floats * 4, hipGetErrorString(e));
        if (p->k) (void)hipFree(p->k);
        if (p->v) (void)hipFree(p->v);
        delete p;
        return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
    }
    *out = p;
    return L2Z_OK;
}

extern "C" int l2z_kvpool_free(l2z_kvpool *p)
{
    if (p == nullptr) return L2Z_OK;
    L2Z_CHECK(p->live == 0, L2Z_ERR_STATE, "l2z_kvpool_free: %d runstates made from the pool are alive", p->live);
    (void)hipSetDevice(p->device);
    (void)hipFree(p->k);
    (void)hipFree(p->v);
    delete p;
    return L2Z_OK;
}

extern "C" int l2z_kvpool_info(const l2z_kvpool *p, int *n_pages, int *n_free, uint64_t *page_bytes)
{
    L2Z_CHECK(p != nullptr, L2Z_ERR_INVALID, "l2z_kvpool_info: null pool");
    if (n_pages) *n_pages = p->alloc.n_pages();
    if (n_free) *n_free = p->alloc.n_free();
    if (page_bytes) *page_bytes = (uint64_t)p->page_floats * 2 * 4;   // keys and values
    return L2Z_OK;
}

extern "C" int l2z_runstate_pages(const l2z_runstate *s, int *n_attached, int32_t *page_ids, int cap)
{
    L2Z_CHECK(s != nullptr, L2Z_ERR_INVALID, "l2z_runstate_pages: null runstate");
    L2Z_CHECK(s->pool != nullptr, L2Z_ERR_INVALID, "l2z_runstate_pages: not a paged runstate");
    L2Z_CHECK(cap >= 0 && (cap == 0 || page_ids != nullptr), L2Z_ERR_INVALID, "l2z_runstate_pages: bad arguments");
    if (n_attached) *n_attached = s->pg.n_attached();
    for (int p = 0; p < cap; p++) page_ids[p] = (size_t)p < s->pg.pages.size() ? s->pg.pages[(size_t)p] : -1;
    return L2Z_OK;
}

extern "C" int l2z_runstate_trim(l2z_runstate *s, int n_pos)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(s != nullptr, L2Z_ERR_INVALID, "l2z_runstate_trim: null runstate");
    L2Z_CHECK(s->pool != nullptr, L2Z_ERR_INVALID, "l2z_runstate_trim: not a paged runstate");
    L2Z_CHECK(n_pos >= 0 && n_pos <= s->cfg.seq_len, L2Z_ERR_STATE, "l2z_runstate_trim: n_pos = %d outside [0, %d]", n_pos,
              s->cfg.seq_len);
    return kv_release(s, n_pos);
}
