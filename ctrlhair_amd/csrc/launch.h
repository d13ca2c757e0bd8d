// launch.h -- host-side launch helpers shared by every launcher: the CU count of the current device, and "once per (kernel, device):
// raise the kernel's dynamic-LDS limit".  Host only; a process may own handles on several GPUs, so both are kept per device index.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

namespace chk {

constexpr int LAUNCH_MAX_DEVICES = 64;

// CU count of device `dev`; 256 when the query fails or the index is outside the cache
inline int device_cus(int dev) {
    static std::atomic<int> cus[LAUNCH_MAX_DEVICES] = {};
    if (dev < 0 || dev >= LAUNCH_MAX_DEVICES) return 256;
    int v = cus[dev].load(std::memory_order_relaxed);
    if (!v) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}
// ... of the current device
inline int device_cus() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? device_cus(dev) : 256;
}

// grid of a persistent launch: one block per CU, fewer when there are fewer tasks
inline int persistent_grid(int ntasks, int cus) { return ntasks < cus ? ntasks : cus; }
inline int persistent_grid(int ntasks) { return persistent_grid(ntasks, device_cus()); }

// hipFuncAttributeMaxDynamicSharedMemorySize = bytes for every kernel of the list, once per device (one flag per list: kernels that a
// first call sets together stay together, which a graph capture after one warm-up call relies on).  `bytes` must be a constant of the
// kernels: the flag does not know it, so a second byte count for the same list would never be set.  hipErrorInvalidDevice when there is
// no current device or its index is outside the flags, otherwise hipFuncSetAttribute's error.  Two threads may both set the attribute:
// harmless, hence relaxed flags and no lock.  `cus` (optional) receives device_cus() of the same device: launchers that size a
// persistent grid ask the runtime for the current device once per launch, not twice.
template <auto... Kernels>
inline hipError_t dyn_lds(int bytes, int* cus = nullptr) {
    static std::atomic<bool> done[LAUNCH_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= LAUNCH_MAX_DEVICES) return hipErrorInvalidDevice;
    if (!done[dev].load(std::memory_order_relaxed)) {
        hipError_t e = hipSuccess;
        ((e = e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(Kernels), hipFuncAttributeMaxDynamicSharedMemorySize, bytes)), ...);
        if (e != hipSuccess) return e;
        done[dev].store(true, std::memory_order_relaxed);
    }
    if (cus) *cus = device_cus(dev);
    return hipSuccess;
}

}  // namespace chk
