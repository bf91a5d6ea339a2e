// Everything the engine gets from the HIP runtime and has to give back, as move-only owners: the two memory policies of host/owned.hpp (device and pinned),
// an event and a stream.  Each counts what is alive in the process (live_resources(), bpg_test_live_resources): relaxed atomics, touched only beside a HIP
// allocation or handle call.  None of these may have static storage duration: a hipFree after the runtime has shut down aborts the process at exit.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <string>
#include <utility>
#include "engine.hpp"
#include "host/owned.hpp"

namespace bpg {

#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw DeviceError(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

enum LiveCounter { LIVE_DEV_BUFS, LIVE_DEV_BYTES, LIVE_PIN_BUFS, LIVE_PIN_BYTES, LIVE_STREAMS, LIVE_EVENTS, LIVE_COUNT };
inline std::atomic<uint64_t> g_live[LIVE_COUNT];
inline void live_add(LiveCounter bufs, LiveCounter bytes, size_t n) { g_live[bufs].fetch_add(1, std::memory_order_relaxed); g_live[bytes].fetch_add(n, std::memory_order_relaxed); }
inline void live_sub(LiveCounter bufs, LiveCounter bytes, size_t n) { g_live[bufs].fetch_sub(1, std::memory_order_relaxed); g_live[bytes].fetch_sub(n, std::memory_order_relaxed); }

struct DeviceMem {
    static void *alloc(size_t bytes) { void *p = nullptr; HIPCHK(hipMalloc(&p, bytes)); live_add(LIVE_DEV_BUFS, LIVE_DEV_BYTES, bytes); return p; }
    static int free(void *p, size_t bytes) { live_sub(LIVE_DEV_BUFS, LIVE_DEV_BYTES, bytes); return (int)hipFree(p); }
};
struct PinnedMem {
    static void *alloc(size_t bytes) { void *p = nullptr; HIPCHK(hipHostMalloc(&p, bytes, hipHostMallocDefault)); live_add(LIVE_PIN_BUFS, LIVE_PIN_BYTES, bytes); return p; }
    static int free(void *p, size_t bytes) { live_sub(LIVE_PIN_BUFS, LIVE_PIN_BYTES, bytes); return (int)hipHostFree(p); }
};
using DevBuf = Owned<DeviceMem>;
using PinBuf = Owned<PinnedMem>;

// A HIP handle with one owner; empty until one of the named constructors made it.  Converts to the raw handle, so it goes wherever the runtime takes one.
template <class H, hipError_t (*Destroy)(H), LiveCounter Counter> class Handle {
    H h = nullptr;
public:
    Handle() = default;
    explicit Handle(H made) : h(made) { g_live[Counter].fetch_add(1, std::memory_order_relaxed); }      // takes over a handle the runtime has just made
    ~Handle() { reset(); }
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    void reset() { if (h) { (void)Destroy(h); g_live[Counter].fetch_sub(1, std::memory_order_relaxed); h = nullptr; } }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy, LIVE_EVENTS> {
    using Handle::Handle;
    static Event timed() { hipEvent_t e; HIPCHK(hipEventCreate(&e)); return Event(e); }
    static Event untimed() { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return Event(e); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy, LIVE_STREAMS> {
    using Handle::Handle;
    static Stream blocking() { hipStream_t s; HIPCHK(hipStreamCreate(&s)); return Stream(s); }                                    // synchronises with the null stream, as hipStreamCreate's do
    static Stream non_blocking() { hipStream_t s; HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return Stream(s); }
};

}  // namespace bpg
