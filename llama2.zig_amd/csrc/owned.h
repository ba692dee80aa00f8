// owned.h -- who frees a scratch buffer, and how a family of them grows.  Nothing of HIP is named here:
// the two raw functions are defined once by the product (runstate.cpp, over hipMalloc / hipHostMalloc / hipFree /
// hipHostFree) and by the host check of this header over malloc (tests/owned_check.cpp).
#pragma once
#include <cstddef>
#include <initializer_list>

namespace l2z {

enum class Mem { Device, Pinned };
// 0 and *p the allocation, or an error code (out of memory: L2Z_ERR_OOM) with *p null and the message set: `what`, the bytes
int raw_alloc(Mem kind, void **p, size_t bytes, const char *what);
void raw_free(Mem kind, void *p);

// One allocation and its owner: null by default, freed with the owner, moved but never copied.  It reads as the T * it
// holds, so only the sites that allocate know the type.
template <class T, Mem K = Mem::Device> class Owned {
  public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset()
    {
        if (p_ != nullptr) raw_free(K, p_);
        p_ = nullptr;
    }
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }
    T *operator->() const { return get(); }
    // make if absent (the buffers a call allocates on its first use and keeps)
    int make(size_t bytes, const char *what) { return p_ != nullptr ? 0 : raw_alloc(K, &p_, bytes, what); }

  private:
    friend struct GrowItem;
    void *p_ = nullptr;
};
template <class T> using Pinned = Owned<T, Mem::Pinned>;

// A member of a group for grow(): the owner and the bytes it takes at the capacity asked for (0: the group has no such
// member at this shape; it stays null)
struct GrowItem {
    template <class T, Mem K> GrowItem(Owned<T, K> &o, size_t bytes) : slot(&o.p_), kind(K), bytes(bytes) {}
    void **slot;
    Mem kind;
    size_t bytes;
};

inline int round_cap(int need, int step) { return (int)(((size_t)need + (size_t)step - 1) / (size_t)step * (size_t)step); }

// every member freed, and the capacity and the key "none"
inline void drop(int *cap, int *key, std::initializer_list<GrowItem> items)
{
    for (const GrowItem &it : items) {
        if (*it.slot != nullptr) raw_free(it.kind, *it.slot);
        *it.slot = nullptr;
    }
    *cap = 0;
    if (key != nullptr) *key = 0;
}

// The one rule by which a group of owners sized by one capacity (and, key != null, made for one key: a group size, a slab
// width) is there for a call.  *cap >= need at an equal key: nothing happens.  Otherwise drain() -- the caller's wait for
// whatever still reads the group; non-zero ends the call --, then every member is freed and every one with a size
// allocated again in list order, the sizes being the caller's for round_cap(need, step).  All or nothing: a failure leaves
// the group empty with the capacity and the key "none" and returns raw_alloc's code; only after the last member stands
// are the rounded capacity and the key recorded.  *remade: whether the members are new (the caller's zero-fills)
template <class Drain>
int grow(const char *what, int *cap, int need, int step, int *key, int want_key, Drain &&drain,
         std::initializer_list<GrowItem> items, bool *remade = nullptr)
{
    if (remade != nullptr) *remade = false;
    if (*cap >= need && (key == nullptr || *key == want_key)) return 0;
    if (const int rc = drain()) return rc;
    drop(cap, key, items);
    for (const GrowItem &it : items) {
        if (it.bytes == 0) continue;
        if (const int rc = raw_alloc(it.kind, it.slot, it.bytes, what)) {
            drop(cap, key, items);
            return rc;
        }
    }
    *cap = round_cap(need, step);
    if (key != nullptr) *key = want_key;
    if (remade != nullptr) *remade = true;
    return 0;
}

}  // namespace l2z
