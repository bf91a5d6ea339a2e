// One owning buffer for every kind of memory the engine allocates (no HIP in here: the engine supplies the policies, tests/hostcheck/owned.cpp a malloc one).
//   Mem::alloc(bytes) -> pointer, throws on failure;  Mem::free(pointer, bytes) -> status, ignored (the capacity travels along for the policy's byte count).
// Move-only: a buffer has exactly one owner, and whoever only reads it holds a plain pointer.
#pragma once
#include <cstddef>
#include <utility>

namespace bpg {

template <class Mem> class Owned {
public:
    void *p = nullptr; size_t cap = 0;      // read them; only ensure(), release() and moves change them
    Owned() = default;
    ~Owned() { release(); }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    // at least `bytes`: a buffer that has to grow is freed FIRST (the peak stays at the larger size; a device free also waits for the device), its contents are lost
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        release();
        p = Mem::alloc(bytes); cap = bytes;
    }
    void release() { if (p) { (void)Mem::free(p, cap); p = nullptr; cap = 0; } }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

}  // namespace bpg
