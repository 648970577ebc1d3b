// device_memory.h -- who owns a device allocation, for every translation unit that makes one (host code only: nothing here is compiled for the device).
// One rule for an allocation (alloc), one owner of a single allocation (Mem), one owner of the allocations of a single call (Temps), and the two small
// helpers every host driver had a copy of (clean, blocks_for).  The frame's and the pipes' DevBuf lists, Scene's fields, query::Scratch and FoldAdapt's
// hand-over keep their own owners.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace dev
{
// no launch or runtime error is pending (and none is left pending)
inline bool clean() { return hipGetLastError() == hipSuccess; }
// blocks of `per` lanes that cover n elements (no overflow at any n)
inline uint32_t blocks_for(size_t n, uint32_t per) { return (uint32_t)(n / per + (n % per != 0u ? 1u : 0u)); }

// THE allocation rule: a request of 0 bytes becomes 16, and a failure returns nullptr with no HIP error left pending.  Where a kernel reads a whole 16-byte
// piece at an array's last element (refit.hip, device_fold.hip) the caller asks for that tail: `count * sizeof(T) + 16`.
inline void* alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
// for a state that keeps typed raw pointers (refit::State, pose::State): p = alloc(bytes) / p freed and cleared
template <class T> bool get(T*& p, size_t bytes) { p = (T*)alloc(bytes); return p != nullptr; }
template <class T> void drop(T*& p) { if (p) (void)hipFree(p); p = nullptr; }

// One allocation and its owner (move-only): freed when the holder goes, unless release() has handed it on.  Nothing is waited for: the holder outlives the
// work that reads it, or that work's stream has been waited for.
struct Mem
{
    Mem() = default;
    explicit Mem(void* owned) : p(owned) {}
    Mem(Mem&& o) noexcept : p(o.release()) {}
    Mem& operator=(Mem&& o) noexcept { if (this != &o) { drop(p); p = o.release(); } return *this; }
    Mem(const Mem&) = delete; Mem& operator=(const Mem&) = delete;
    ~Mem() { drop(p); }
    bool alloc(size_t bytes) { drop(p); return dev::get(p, bytes); }
    void free() { drop(p); }
    // src's `bytes` into the allocation, on `stream` (nothing to do without a source); false: the copy failed
    bool upload(hipStream_t stream, const void* src, size_t bytes) const { return !src || bytes == 0 || hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess; }
    template <class T = void> T* get() const { return (T*)p; }
    explicit operator bool() const { return p != nullptr; }
    void* release() { void* q = p; p = nullptr; return q; }
private:
    void* p = nullptr;
};

// The allocations of one call, freed together.  The destructor WAITS FOR THE STREAM before it frees (when it holds anything), so a user may return on any
// path, a launch still in flight included; after finish() or a wait of the user's own that wait finds the stream idle.
struct Temps
{
    // tail: bytes added to every allocation (see alloc)
    explicit Temps(hipStream_t s, size_t tail_bytes = 0) : stream(s), tail(tail_bytes) {}
    Temps(const Temps&) = delete; Temps& operator=(const Temps&) = delete;
    ~Temps()
    {
        if (!held.empty()) (void)hipStreamSynchronize(stream);
        for (void* p : held) if (p) (void)hipFree(p);
    }
    // a new allocation, `src` uploaded into it when there is one.  nullptr: the allocation or the upload failed
    void* get(const void* src, size_t bytes)
    {
        void* p = alloc(bytes + tail);
        if (!p) return nullptr;
        held.push_back(p);
        return !src || bytes == 0 || hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess ? p : nullptr;
    }
    // the same for `count` elements of T, nothing uploaded
    template <class T> bool array(T*& out, size_t count) { out = (T*)get(nullptr, count * sizeof(T)); return out != nullptr; }
    // p leaves the set: the caller owns it now
    template <class T> T* keep(T* p) { for (void*& q : held) if (q == p) q = nullptr; return p; }
    // after the launch: d_out's `bytes` to `out`, the stream waited for.  launched: what clean() said after the launch
    bool finish(bool launched, void* out, const void* d_out, size_t bytes)
    {
        bool ok = launched && hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
        ok = hipStreamSynchronize(stream) == hipSuccess && ok;
        (void)hipGetLastError();
        return ok;
    }
private:
    hipStream_t stream;
    size_t tail;
    std::vector<void*> held;
};
} // namespace dev
