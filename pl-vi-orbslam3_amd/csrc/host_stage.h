// host_stage.h — the staging of a synchronous "one item from host memory"
// entry point.  The entry point declares each array once, typed, as rows of
// `width` elements; commit() makes ONE zero-filled device block of
// 256-byte-aligned slots and uploads the inputs, dev() gives the typed device
// pointers for the _batch call, and fetch() waits and downloads the outputs.
#pragma once
#include <algorithm>
#include <functional>
#include <type_traits>
#include <vector>

#include "plvi_common.h"

namespace plvi {

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

// A declared array.  The default one is absent: dev() gives nullptr, which is
// how a NULL optional of the host form reaches the _batch form unchanged.
template <class T>
struct Staged {
    int i = -1;
};

class HostStage {
  public:
    // Declarations, before commit().  An array is n rows of `width` elements
    // in a slot of max(n, cap, 1) rows: a present array has a distinct
    // non-NULL device address even when empty, and a capacity of max(n, 1)
    // needs no `cap`.  n rows are uploaded; a NULL src is absent ...
    template <class T>
    Staged<T> in(const T* src, size_t n, size_t width = 1, size_t cap = 0) {
        return add<T>(src != nullptr, src, nullptr, n, width, cap);
    }
    // ... or present and all zero (a required array of an empty side, NULL `blocked`)
    template <class T>
    Staged<T> in_or_zero(const T* src, size_t n, size_t width = 1, size_t cap = 0) {
        return add<T>(true, src, nullptr, n, width, cap);
    }
    // n rows are downloaded by fetch(); a NULL dst is absent ...
    template <class T>
    Staged<T> out(T* dst, size_t n, size_t width = 1) {
        return add<T>(dst != nullptr, nullptr, dst, n, width, 0);
    }
    // ... or present and not downloaded (the _batch form writes it regardless)
    template <class T>
    Staged<T> out_or_scratch(T* dst, size_t n, size_t width = 1) {
        return add<T>(true, nullptr, dst, n, width, 0);
    }
    // uploaded and downloaded; small by-value blocks (counts, params) are an inout of a local array
    template <class T>
    Staged<T> inout(T* p, size_t n, size_t width = 1, size_t cap = 0) {
        return add<T>(p != nullptr, p, p, n, width, cap);
    }
    template <class T>
    Staged<T> scratch(size_t n) {
        return add<T>(true, nullptr, nullptr, n, 1, 0);
    }
    // For a _batch form that takes structs of pointers: work on a copy of the
    // caller's struct and declare each array through the copy's field.  The
    // field holds the host pointer now (NULL is absent); commit() replaces it
    // by the device pointer.
    enum Dir { In = 1, Out = 2, InOut = 3 };
    template <class P>
    Staged<typename std::remove_const<P>::type> field(P*& f, Dir dir, size_t n, size_t width = 1) {
        using T = typename std::remove_const<P>::type;
        T* host = const_cast<T*>(f);
        const Staged<T> s = add<T>(host != nullptr, dir & In ? host : nullptr, dir & Out ? host : nullptr, n, width, 0);
        patches.push_back([this, &f, s] { f = dev(s); });
        return s;
    }

    // The one allocation, the one zero fill and the uploads, all complete on return.
    int commit() {
        if (d.alloc(tot)) return PLVI_E_HIP;
        if (!tot) return PLVI_OK;
        for (const std::function<void()>& patch : patches) patch();
        PLVI_CHECK(hipMemset(d.p, 0, tot));
        for (const Slot& s : slots)
            if (s.up) PLVI_CHECK(hipMemcpy(d.as<uint8_t>() + s.off, s.src, s.up, hipMemcpyHostToDevice));
        PLVI_CHECK(hipStreamSynchronize(nullptr));  // the fill too, for a _batch call on a non-blocking stream
        return PLVI_OK;
    }
    template <class T>
    T* dev(Staged<T> s) const {  // after commit()
        return s.i < 0 ? nullptr : reinterpret_cast<T*>(d.as<uint8_t>() + slots[s.i].off);
    }

    // Download only the first n rows (a count known after the run); never more than declared.
    template <class T>
    void trim(Staged<T> s, size_t n, size_t width = 1) {
        if (s.i >= 0) slots[s.i].down = std::min(slots[s.i].down, n * width * sizeof(T));
    }
    // Wait (for the stream if one is given, else for the device) and download
    // every output not fetched yet; fetch_one() downloads one slot alone, for
    // the counts that trim() needs.
    int fetch(hipStream_t st = nullptr) {
        if (int rc = wait(st)) return rc;
        for (Slot& s : slots)
            if (int rc = pull(s)) return rc;
        return PLVI_OK;
    }
    template <class T>
    int fetch_one(Staged<T> s, hipStream_t st = nullptr) {
        if (int rc = wait(st)) return rc;
        return s.i < 0 ? PLVI_OK : pull(slots[s.i]);
    }

  private:
    struct Slot {
        size_t off;
        const void* src;
        size_t up;  // bytes to upload
        void* dst;
        size_t down;  // bytes still to download
    };
    std::vector<Slot> slots;
    std::vector<std::function<void()>> patches;  // field(): host pointer -> device pointer
    size_t tot = 0;
    DevBuf d;

    template <class T>
    Staged<T> add(bool present, const T* src, T* dst, size_t n, size_t width, size_t cap) {
        if (!present) return {};
        const size_t row = width * sizeof(T);
        slots.push_back({tot, src, src ? n * row : 0, dst, dst ? n * row : 0});
        tot += up256(std::max(std::max({n, cap, size_t(1)}) * row, size_t(1)));
        return {(int)slots.size() - 1};
    }
    static int wait(hipStream_t st) {
        PLVI_CHECK(st ? hipStreamSynchronize(st) : hipDeviceSynchronize());
        return PLVI_OK;
    }
    int pull(Slot& s) {
        if (s.down) PLVI_CHECK(hipMemcpy(s.dst, d.as<uint8_t>() + s.off, s.down, hipMemcpyDeviceToHost));
        s.down = 0;
        return PLVI_OK;
    }
};

}  // namespace plvi
