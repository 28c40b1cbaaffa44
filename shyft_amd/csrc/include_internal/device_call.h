// Internal, host-only: what the stateless batched entries (shyft_hip_kalman_run, _quantile_map, _resample, the
// shyft_hip_ts_* entries, _forecast_skill, shyft_hip_btk, shyft_hip_ordinary_kriging) share on the host side of one device call.
#pragma once
#include <atomic>
#include <string>

#include "region_impl.h"

namespace shyft_hip_impl {

// The stream and the two events of one device call. A timed call is
//   upload ..; begin(); launch ..; end(); download ..; ms = finish(what);
// so the events bracket the kernels and the copies stay outside. An untimed call leaves begin() and end() out.
struct device_call {
    int dev = 0;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit device_call(int device) {
        if (device >= 0) hip_check(hipSetDevice(device), "hipSetDevice");
        hip_check(hipGetDevice(&dev), "hipGetDevice");
        hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            release();
            throw std::runtime_error("hipEventCreate failed");
        }
    }
    device_call(const device_call&) = delete;
    device_call& operator=(const device_call&) = delete;
    ~device_call() { release(); }
    void release() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
        e0 = e1 = nullptr;
        s = nullptr;
    }
    // a count of 0 leaves d.p == nullptr
    template <class T>
    void upload(dbuf<T>& d, const T* src, size_t count, const char* what) {
        d.alloc(count);
        if (count) hip_check(hipMemcpyAsync(d.p, src, count * sizeof(T), hipMemcpyHostToDevice, s), what);
    }
    template <class T>
    void download(T* dst, const T* d_src, size_t count, const char* what) {
        hip_check(hipMemcpyAsync(dst, d_src, count * sizeof(T), hipMemcpyDeviceToHost, s), what);
    }
    void begin() { hip_check(hipEventRecord(e0, s), "hipEventRecord"); }
    void end() { hip_check(hipEventRecord(e1, s), "hipEventRecord"); }
    void sync(const char* what) { hip_check(hipStreamSynchronize(s), what); }
    // waits for the stream; the milliseconds between begin() and end()
    double finish(const char* what) {
        sync(what);
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
        return double(ms);
    }
};

// One value per device ordinal (the last kernel time, a call count, the last launch shape), zero until stored.
template <class T>
struct per_device {
    static constexpr int MAX_DEVICES = 64;
    std::atomic<T> v[MAX_DEVICES];
    static bool in_range(int dev) { return dev >= 0 && dev < MAX_DEVICES; }
    void store(int dev, T x) {
        if (in_range(dev)) v[dev].store(x);
    }
    T fetch_add(int dev, T x) { return in_range(dev) ? v[dev].fetch_add(x) : T(); }
    // device < 0 is the current device; fallback when that cannot be read or the ordinal is out of range
    T load(int device, T fallback) const {
        if (device < 0 && hipGetDevice(&device) != hipSuccess) return fallback;
        return in_range(device) ? v[device].load() : fallback;
    }
};

// The grid of a kernel whose stride loop takes what the grid does not: at least one block, at most 2^20.
inline unsigned launch_blocks(size_t blocks) {
    const size_t max_grid = size_t(1) << 20;
    return unsigned(blocks < max_grid ? (blocks ? blocks : 1) : max_grid);
}

// What the getters of one entry family report per device: the kernel milliseconds of the last call, the calls so far
// and the last launch shape. A family without a shape or a call getter leaves that member unread.
struct call_record {
    static constexpr int KEEP_PATH = -0x7fffffff - 1;
    per_device<double> last_ms;
    per_device<uint64_t> calls;
    per_device<int> last_path;
    // the counters alone, for an entry that downloads several arrays or adds up the times of several launches
    void record(int dev, double ms, int path = KEEP_PATH) {
        last_ms.store(dev, ms);
        calls.fetch_add(dev, 1);
        if (path != KEEP_PATH) last_path.store(dev, path);
    }
    // after the last launch of a timed call with one result array: the end of the timed part, the result, the wait,
    // and the counters
    template <class T>
    void finish(device_call& c, const char* what, T* out, const T* d_out, size_t count, int path = KEEP_PATH) {
        c.end();
        c.download(out, d_out, count, (std::string(what) + " download").c_str());
        record(c.dev, c.finish(what), path);
    }
};

}  // namespace shyft_hip_impl
