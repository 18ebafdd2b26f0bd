// host_stage.h — the staging of a synchronous single-pair entry point: one
// device block of 256-byte-aligned slots, filled from host arrays, and the
// sync + download tail.
#pragma once
#include <vector>

#include "plvi_common.h"

namespace plvi {

struct HostStage {
    std::vector<size_t> off;
    size_t tot = 0;
    DevBuf d;

    size_t put(size_t bytes) {  // reserve a slot (before alloc)
        off.push_back(tot);
        tot += (bytes + 255) & ~size_t(255);
        return off.size() - 1;
    }
    int alloc(bool zero_fill = false) {
        if (d.alloc(tot)) return PLVI_E_HIP;
        if (zero_fill) PLVI_CHECK(hipMemset(d.p, 0, tot));
        return PLVI_OK;
    }
    template <class T>
    T* at(size_t slot) const {
        return reinterpret_cast<T*>(d.as<uint8_t>() + off[slot]);
    }
    int up(size_t slot, const void* src, size_t bytes) const {  // a NULL or empty source is skipped
        if (src && bytes) PLVI_CHECK(hipMemcpy(at<void>(slot), src, bytes, hipMemcpyHostToDevice));
        return PLVI_OK;
    }
    int up_or_zero(size_t slot, const void* src, size_t bytes) const {  // a NULL source = all zero
        if (!src) PLVI_CHECK(hipMemset(at<void>(slot), 0, bytes));
        return up(slot, src, bytes);
    }
    // The shared tail: wait for the kernels, download the n (n_r) entries of
    // the match table(s), return the device count *d_count or an error.
    int finish(const int* d_count, int* match, size_t m_slot, int n, int* match_r = nullptr, size_t r_slot = 0,
               int n_r = 0) const {
        PLVI_CHECK(hipDeviceSynchronize());
        int count = 0;
        if (n) PLVI_CHECK(hipMemcpy(match, at<void>(m_slot), 4 * (size_t)n, hipMemcpyDeviceToHost));
        if (n_r) PLVI_CHECK(hipMemcpy(match_r, at<void>(r_slot), 4 * (size_t)n_r, hipMemcpyDeviceToHost));
        PLVI_CHECK(hipMemcpy(&count, d_count, 4, hipMemcpyDeviceToHost));
        return count;
    }
};

}  // namespace plvi
