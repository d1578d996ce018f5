// kf_devbuf.hpp -- DevBuf<T>: the one owner of a raw block of device memory above the C ABI.  Move-only; remembers {ctx, pointer, bytes} and frees with the ctx the block
// was allocated with.  Calls kf_malloc, kf_tp_alloc, kf_free and kf_memset and nothing else of the ABI (tests/devbuf_main.cpp stands in for those four on the host).
#pragma once
#include <cstddef>

#include "../../include/kf_abi.h"

namespace koifish {

template <class T = void>
class DevBuf {
    kf_ctx* ctx_ = nullptr;
    T* p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) Free(), ctx_ = o.ctx_, p_ = o.p_, bytes_ = o.bytes_, o.p_ = nullptr, o.bytes_ = 0;
        return *this;
    }
    ~DevBuf() { Free(); }
    // frees what is held, then allocates; on failure the buffer is empty.  uncached: kf_tp_alloc, a receive area peers may map (zeroed by the ABI)
    int Alloc(kf_ctx* c, size_t bytes, bool uncached = false) {
        Free();
        void* p = nullptr;
        const int rc = uncached ? kf_tp_alloc(c, bytes, &p) : kf_malloc(c, bytes, &p);
        if (rc == KF_OK) ctx_ = c, p_ = static_cast<T*>(p), bytes_ = bytes;
        return rc;
    }
    int AllocUncached(kf_ctx* c, size_t bytes) { return Alloc(c, bytes, true); }
    int AllocFilled(kf_ctx* c, size_t bytes, int byte = 0) {  // ... and every byte set (on the ctx's stream)
        int rc = Alloc(c, bytes);
        if (rc == KF_OK && (rc = kf_memset(c, p_, byte, bytes)) != KF_OK) Free();
        return rc;
    }
    void Free() {
        if (p_) kf_free(ctx_, p_);
        p_ = nullptr, bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }  // 0 when empty
    T* get() const { return p_; }
    operator T*() const { return p_; }  // so that `d_state + 4 * s` and kf_* arguments read as with a raw pointer
    explicit operator bool() const { return p_ != nullptr; }
};

}  // namespace koifish
