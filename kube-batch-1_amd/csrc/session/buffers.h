// buffers.h — the RAII holders of a session's pooled memory: DevBuf (device
// memory) and PinnedBuf (pinned host staging).  Part of session.h, which
// includes it after what it uses: MemPool, Error, HIPCHK and the HIP runtime's
// hipGetDevice / hipStreamSynchronize.  It names nothing else, so that a
// stand-alone host program can compile it against stand-ins for those.
#pragma once

namespace kbhip {

struct DevBuf {  // device memory (pooled), or host memory for encode-only sessions
    void* p = nullptr;
    bool host = false;
    size_t cap = 0;  // the block's size (the pool may hand out up to twice what was asked for)
    size_t req = 0;  // the bytes asked for
    int dev = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) { if (host) std::free(p); else MemPool::get().give(MemPool::kDevice, p, cap, dev); }
        p = nullptr;
        req = 0;
    }
    template <typename T>
    T* alloc(size_t n, bool on_host = false) {
        release();
        host = on_host;
        size_t bytes = std::max<size_t>(n * sizeof(T), 16);
        if (host) {
            p = std::calloc(1, bytes);
            if (!p) throw Error(KBHIP_EINVAL, "out of host memory");
        } else {
            (void)hipGetDevice(&dev);
            p = MemPool::get().take(MemPool::kDevice, bytes, &cap);
        }
        req = bytes;
        return (T*)p;
    }
    // A buffer that work queued on `stream` reads and that only grows: nothing while it holds need_bytes
    // of what was asked for; else alloc_bytes (the caller's growth policy) once the stream has drained —
    // the old block goes back to the pool, whose next taker must not meet its last reader.
    void grow(hipStream_t stream, size_t need_bytes, size_t alloc_bytes) {
        if (p && req >= need_bytes) return;
        if (p) HIPCHK(hipStreamSynchronize(stream));
        alloc<uint8_t>(std::max(need_bytes, alloc_bytes));
    }
};

struct PinnedBuf {  // pinned host memory (pooled, MemPool::kPinned) of the device it was taken on
    void* p = nullptr;
    size_t cap = 0;
    int dev = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    void release() {
        if (p) MemPool::get().give(MemPool::kPinned, p, cap, dev);
        p = nullptr;
        cap = 0;
    }
    // Nothing while the block holds need_bytes; else the block goes back and one of alloc_bytes (the
    // caller's growth policy) is taken.  The caller knows that no copy still reads or writes the old one.
    void fit(size_t need_bytes, size_t alloc_bytes) {
        if (p && cap >= need_bytes) return;
        release();
        (void)hipGetDevice(&dev);
        p = MemPool::get().take(MemPool::kPinned, std::max(need_bytes, alloc_bytes), &cap);
    }
    void fit(size_t bytes) { fit(bytes, bytes); }
    template <typename T>
    T* as() const { return (T*)p; }
};

}  // namespace kbhip
