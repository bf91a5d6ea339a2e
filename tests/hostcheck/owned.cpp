// TEST HARNESS, stand-alone: the owning buffer of the engine (csrc/host/owned.hpp) through the host compiler, on a malloc policy that counts what is alive,
// logs every call in order and can be told to fail the next allocation.  tests/test_owned_host.py builds it with -fsanitize=address,undefined and expects "ok"
// on the last line; ASan's leak check at exit backs the policy's own count.
#include "../../bulletproofs_gadgets_amd/csrc/host/owned.hpp"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <vector>
using namespace bpg;

struct CountingMem {
    static inline long blocks = 0, bytes = 0;
    static inline bool fail_next = false;
    static inline std::string log;                      // 'a' per allocation, 'f' per free, in call order
    static void *alloc(size_t n) {
        log += 'a';
        if (fail_next) { fail_next = false; throw std::bad_alloc(); }
        void *p = std::malloc(n);
        if (!p) throw std::bad_alloc();
        blocks++; bytes += (long)n;
        return p;
    }
    static int free(void *p, size_t n) { log += 'f'; blocks--; bytes -= (long)n; std::free(p); return 0; }
};
using Buf = Owned<CountingMem>;
using M = CountingMem;

static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "a buffer has one owner");
static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "containers move buffers, they never copy them");

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
static bool live(long blocks, long bytes) { return M::blocks == blocks && M::bytes == bytes; }

int main() {
    {   // ensure within capacity makes no call; growth frees before it allocates; release twice
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0);
        b.ensure(0); CHECK(M::log.empty() && b.p == nullptr);
        b.ensure(100); CHECK(M::log == "a" && b.p && b.cap == 100 && live(1, 100));
        void *p0 = b.p;
        b.as<uint8_t>()[99] = 7;
        b.ensure(100); b.ensure(40); b.ensure(1); CHECK(M::log == "a" && b.p == p0 && b.cap == 100);
        b.ensure(101); CHECK(M::log == "afa" && b.cap == 101 && live(1, 101));
        b.as<uint8_t>()[100] = 7;
        b.release(); CHECK(M::log == "afaf" && b.p == nullptr && b.cap == 0 && live(0, 0));
        b.release(); CHECK(M::log == "afaf");
    }
    CHECK(M::log == "afaf" && live(0, 0));                // the destructor of an empty buffer makes no call
    M::log.clear();
    {   // a failing allocation throws and leaves the buffer empty - also when it held memory before - and a later ensure works
        Buf b;
        M::fail_next = true;
        bool threw = false;
        try { b.ensure(64); } catch (const std::bad_alloc &) { threw = true; }
        CHECK(threw && b.p == nullptr && b.cap == 0 && live(0, 0));
        b.ensure(64); CHECK(b.p && b.cap == 64 && live(1, 64));
        M::fail_next = true; threw = false;
        try { b.ensure(128); } catch (const std::bad_alloc &) { threw = true; }
        CHECK(threw && b.p == nullptr && b.cap == 0 && live(0, 0) && M::log == "aafa");
        b.ensure(16); CHECK(b.cap == 16 && live(1, 16));
    }
    CHECK(live(0, 0));
    M::log.clear();
    {   // moves: construction, assignment onto a non-empty target, self-move
        Buf a; a.ensure(10);
        void *pa = a.p;
        Buf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 10 && live(1, 10) && M::log == "a");
        Buf c; c.ensure(20); CHECK(live(2, 30));
        c = std::move(b);
        CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 10 && live(1, 10) && M::log == "aaf");
        Buf &alias = c;
        c = std::move(alias);
        CHECK(c.p == pa && c.cap == 10 && live(1, 10) && M::log == "aaf");
        c = Buf(); CHECK(c.p == nullptr && live(0, 0));    // assignment from an empty buffer frees the target
    }
    CHECK(live(0, 0));
    M::log.clear();
    {   // a vector that reallocates moves its buffers: same pointers, nothing freed
        std::vector<Buf> v(2);
        v[0].ensure(8); v[1].ensure(9);
        void *p0 = v[0].p, *p1 = v[1].p;
        const Buf *where = v.data();
        v.resize(v.capacity() + 50);
        CHECK(v.data() != where);                          // it did reallocate
        CHECK(v[0].p == p0 && v[1].p == p1 && v[0].cap == 8 && v[1].cap == 9 && v[2].p == nullptr && M::log == "aa" && live(2, 17));
        v.resize(1); CHECK(M::log == "aaf" && live(1, 8));
    }
    CHECK(live(0, 0));
    M::log.clear();
    {   // a map takes its tables by move and frees them with itself; what is handed out afterwards is read from the entry
        std::map<uint32_t, Buf> m;
        Buf t; t.ensure(32);
        void *pt = t.p;
        const uint8_t *view = (m[5] = std::move(t)).as<uint8_t>();
        CHECK(view == pt && t.p == nullptr && m[5].cap == 32 && live(1, 32));
        Buf u; u.ensure(48);
        m.emplace(7u, std::move(u));
        CHECK(u.p == nullptr && m.size() == 2 && live(2, 80));
        m.erase(5); CHECK(live(1, 48));
    }
    CHECK(live(0, 0));
    if (failures) { std::printf("FAILED: %d checks\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
