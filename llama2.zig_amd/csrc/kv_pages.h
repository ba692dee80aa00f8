// kv_pages.h -- the host bookkeeping of the paged KV cache (include/llama2_hip_test.h l2z_kvpool; device side:
// kv_pool.cpp): which pages of a pool are free, how many sequences hold each one, and every sequence's page table.
// Plain C++ with no HIP in it, so a stand-alone program can test it (tests/test_kv_pages_host.py).
//
// A page is kKvPage consecutive positions; page p of a sequence covers positions kKvPage * p .. kKvPage * p + kKvPage - 1.
// Nothing here is thread-safe: a pool and the runstates made from it belong to one host thread at a time, as a runstate does.
#pragma once
#include <cstdint>
#include <vector>

namespace l2z {

constexpr int kKvPage = 64;  // L2Z_KV_PAGE: == kVerifySeg, the segment of the verify / wide attention

inline int kv_pages_for(int n_pos) { return (n_pos + kKvPage - 1) / kKvPage; }

// A sequence's page table: pages[p] = the pool's page that holds positions kKvPage * p .., or -1
struct KvSeq {
    std::vector<int32_t> pages;
    void init(int seq_len) { pages.assign((size_t)kv_pages_for(seq_len), -1); }
    int n_attached() const
    {
        int n = 0;
        for (int32_t p : pages) n += p >= 0;
        return n;
    }
};

// The free list (a stack: the page given back last goes out first; a fresh pool hands out 0, 1, 2, ...) and the
// number of holders of every page
class KvPages {
  public:
    explicit KvPages(int n_pages = 0) { reset(n_pages); }
    void reset(int n_pages)
    {
        refs_.assign((size_t)n_pages, 0);
        free_.resize((size_t)n_pages);
        for (int i = 0; i < n_pages; i++) free_[(size_t)i] = n_pages - 1 - i;
    }
    int n_pages() const { return (int)refs_.size(); }
    int n_free() const { return (int)free_.size(); }
    int refs(int page) const { return refs_[(size_t)page]; }

    // pages of positions [a, b) that s does not hold yet (b <= the positions s was made for)
    int missing(const KvSeq &s, int a, int b) const
    {
        int n = 0;
        if (a < b)
            for (int p = a / kKvPage; p <= (b - 1) / kKvPage; p++) n += s.pages[(size_t)p] < 0;
        return n;
    }
    // some position of [a, b) lies in a page that s holds together with another sequence: a write there is refused
    bool writes_shared(const KvSeq &s, int a, int b) const
    {
        if (a < b)
            for (int p = a / kKvPage; p <= (b - 1) / kKvPage; p++)
                if (s.pages[(size_t)p] >= 0 && refs_[(size_t)s.pages[(size_t)p]] > 1) return true;
        return false;
    }
    // s holds every page of [a, b) afterwards; false, with nothing attached, when the free pages do not suffice
    bool attach(KvSeq &s, int a, int b)
    {
        if (missing(s, a, b) > n_free()) return false;
        if (a < b)
            for (int p = a / kKvPage; p <= (b - 1) / kKvPage; p++)
                if (s.pages[(size_t)p] < 0) {
                    const int32_t id = free_.back();
                    free_.pop_back();
                    refs_[(size_t)id] = 1;
                    s.pages[(size_t)p] = id;
                }
        return true;
    }
    // dst (which holds nothing there) holds src's pages 0 .. n_whole - 1 too; all of them are attached to src
    void share(KvSeq &dst, const KvSeq &src, int n_whole)
    {
        for (int p = 0; p < n_whole; p++) {
            const int32_t id = src.pages[(size_t)p];
            refs_[(size_t)id]++;
            dst.pages[(size_t)p] = id;
        }
    }
    // s lets go of every page that lies wholly at or above n_pos (0: of all); a page goes back to the free list when its
    // last holder lets go.  Returns how many s let go of.
    int release(KvSeq &s, int n_pos = 0)
    {
        int n = 0;
        for (size_t p = (size_t)kv_pages_for(n_pos); p < s.pages.size(); p++) {
            const int32_t id = s.pages[p];
            if (id < 0) continue;
            if (--refs_[(size_t)id] == 0) free_.push_back(id);
            s.pages[p] = -1;
            n++;
        }
        return n;
    }

  private:
    std::vector<int32_t> free_;
    std::vector<int32_t> refs_;
};

}  // namespace l2z
