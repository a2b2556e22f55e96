// devbuf.hpp — the owners of device and pinned host memory.
//
// Every buffer frees itself with whatever holds it: a context's buffers go inside `delete c`, on the thread that set the device,
// after mmp_destroy has stopped what could still read them.  None of these types may stand at namespace or static scope: its
// destructor would run at process exit, after the HIP runtime has gone.
//
// The header uses hipError_t, hipSuccess, hipMalloc, hipFree, hipHostMalloc and hipHostFree and includes nothing that declares them:
// mmplace.hip includes it after <hip/hip_runtime.h>, tests/devbuf_host/devbuf_test.cc after its counting stand-ins.
#pragma once

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // exactly `bytes`, into an empty buffer (the callers with a growth policy of their own; everyone else: ensure)
    hipError_t alloc(size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess)
            cap = bytes;
        else
            p = nullptr;
        return e;
    }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        size_t want = std::max<size_t>(bytes, 256);
        want = (want + 255) & ~size_t(255);
        return alloc(want);
    }
    hipError_t release_checked()  // release, for the caller that reports what hipFree answers
    {
        hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    void release() { (void)release_checked(); }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && std::is_nothrow_move_constructible_v<DevBuf>, "DevBuf is move-only");

// A DevBuf built beside a published one: the carrier of the library's ownership rule (written out at mmp_ctx::mid_hash).  Its
// owner holds batch_mu and declares it ahead of the work; move_into, under the state lock held EXCLUSIVE, publishes it and takes
// what it replaced, which stays allocated and unwritten until this object ends or is released explicitly.  Between the swap and
// that end the owner runs the drain (quiesce_decisions: inside the hold, or behind it), so no kernel that captured the replaced
// buffer is still running when it goes.  Never published: released on every way out, a thrown one included.  Every buffer frees
// itself with its context; ScopedDevBuf is about WHEN a replaced buffer may go.
struct ScopedDevBuf {
    DevBuf b;
    bool move_into(DevBuf &dst)  // whether there was anything to publish
    {
        if (!b.p) return false;
        std::swap(dst, b);
        return true;
    }
    void release() { b.release(); }
};

// Pinned host memory (hipHostMalloc / hipHostFree), `count` elements of T.
template <class T>
struct PinBuf {
    T *p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
    PinBuf &operator=(PinBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
        }
        return *this;
    }
    ~PinBuf() { release(); }
    hipError_t alloc(size_t count, unsigned int flags)  // into an empty buffer
    {
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
};
static_assert(!std::is_copy_constructible_v<PinBuf<int>> && std::is_nothrow_move_constructible_v<PinBuf<int>>, "PinBuf is move-only");
