// owned.hpp — move-only owners of the HIP resources a handle holds: device buffer, pinned host
// buffer, event, stream. A destructor releases what its owner holds, so a handle's destroy function
// only synchronises its streams and deletes the handle. An owner converts to its raw pointer for
// host-side use; it cannot be copied, so a kernel launch (whose argument types are deduced) takes
// .get().
#pragma once

#include <type_traits>
#include <utility>

#include "common.hpp"

namespace gsgpu {

struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreePinned { void operator()(void* p) const { (void)hipHostFree(p); } };
struct FreeEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FreeStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };

template <typename P, typename Free>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (p_) Free{}(std::exchange(p_, nullptr)); }
    P get() const { return p_; }
    operator P() const { return p_; }

protected:
    P p_ = nullptr;
};

struct Event : Owned<hipEvent_t, FreeEvent> {
    int create(unsigned flags = hipEventDisableTiming) {
        reset();
        GS_HIP(hipEventCreateWithFlags(&p_, flags));
        return GS_OK;
    }
};

struct Stream : Owned<hipStream_t, FreeStream> {
    int create() {
        reset();
        GS_HIP(hipStreamCreateWithFlags(&p_, hipStreamNonBlocking));
        return GS_OK;
    }
};

// n elements of pinned host memory (bytes for T = void)
template <typename T = void>
struct Pinned : Owned<T*, FreePinned> {
    int alloc(size_t n, const char* what) {
        this->reset();
        const size_t bytes = n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        if (hipHostMalloc(reinterpret_cast<void**>(&this->p_), bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            this->p_ = nullptr;
            return fail(GS_ERR_NOMEM, "%s: %zu bytes of pinned memory", what, bytes);
        }
        return GS_OK;
    }
};

// Device memory and its capacity in elements (bytes for T = void).
template <typename T = void>
class DevBuf : public Owned<T*, FreeDevice> {
    using Base = Owned<T*, FreeDevice>;
    size_t cap_ = 0;

    int grow_to(size_t need, const char* what, bool drain, hipStream_t s) {
        if (this->p_ && cap_ >= need) return GS_OK;
        if (this->p_ && drain) GS_HIP(hipStreamSynchronize(s));
        reset();
        const size_t bytes = need * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        if (hipMalloc(reinterpret_cast<void**>(&this->p_), bytes) != hipSuccess) {
            (void)hipGetLastError();
            this->p_ = nullptr;
            return fail(GS_ERR_NOMEM, "%s: %zu bytes of device memory", what, bytes);
        }
        cap_ = need;
        return GS_OK;
    }

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : Base(std::move(o)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { Base::operator=(std::move(o)); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    size_t capacity() const { return cap_; }
    void reset() { Base::reset(); cap_ = 0; }
    // Room for `need` elements: nothing to do when the capacity suffices, else the old memory is
    // freed (after the work queued on `drain`, for a buffer that work may still use) and new memory
    // allocated. On failure the buffer is empty with capacity 0, so the next call allocates again.
    int grow(size_t need, const char* what) { return grow_to(need, what, false, nullptr); }
    int grow(size_t need, const char* what, hipStream_t drain) { return grow_to(need, what, true, drain); }
};

// A group of owners created on first use is made whole or not at all: built in a local and moved
// into its place only when every member exists, so a failure leaves `dst` as it was.
template <typename G, typename... A>
int make_whole(G& dst, A&&... a) {
    G g;
    GS_TRY(g.create(std::forward<A>(a)...));
    dst = std::move(g);
    return GS_OK;
}

}  // namespace gsgpu
