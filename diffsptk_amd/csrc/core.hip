// Core entries of the library: its version, the calling thread's error / dispatch record (common.h), the device count and
// the frame count of Frame (frame.py:139) that every framing entry uses.
#include "common.h"

using namespace dsa;

DSA_EXPORT int dsa_version(void) { return DSA_VERSION; }
DSA_EXPORT const char* dsa_last_error(void) { return err_buf(); }
DSA_EXPORT const char* dsa_last_kernel(void) { return kernel_name(); }
DSA_EXPORT int dsa_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(DSA_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}
DSA_EXPORT int64_t dsa_num_frames(int64_t T, int32_t P) { return (T <= 0 || P <= 0) ? 0 : (T - 1) / P + 1; }
