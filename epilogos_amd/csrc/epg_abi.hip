// The parts of libepilogos_hip.so that belong to no kernel: the error message, the device query, the test switches and the
// workspace sizes.  Every other entry point of include/epilogos_amd.h is defined next to its kernels.
#include "epg_common.h"

namespace epg {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int g_force[FORCE_COUNT] = {0};

int num_cus() {
    if (g_force[FORCE_CUS] > 0) return g_force[FORCE_CUS];    // the tests' grid cap: before the cache, so set and reset act at once
    static thread_local int cached_dev = -1;
    static thread_local int cached_cus = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached_dev = dev;
        cached_cus = cus;
    }
    return cached_cus;
}

}  // namespace epg

using namespace epg;

extern "C" {

int epg_test_force(int32_t which, int32_t value) {
    if (which < 0 || which >= FORCE_COUNT) return fail(EPG_ERR_INVALID_ARG, "test_force: unknown switch %d", which);
    g_force[which] = value;
    return EPG_OK;
}

int epg_version(void) { return EPG_ABI_VERSION; }
const char* epg_last_error(void) { return g_err; }

int epg_device_cus(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(EPG_ERR_HIP, "no HIP device available");
    return num_cus();
}

int64_t epg_ws_bytes(int32_t saliency, int64_t R, int32_t N, int32_t S) {
    if (R < 0 || N < 1 || S < 1) return fail(EPG_ERR_INVALID_ARG, "ws_bytes: bad shape");
    switch (saliency) {
        case 1: return s1_ws_bytes(R, N, S);
        case 2: return s2_table_bytes(N, S) + align_up(R * S * 2, 256);
        case 3: return s3_ws_bytes(R, N, S);
        default: return fail(EPG_ERR_INVALID_ARG, "ws_bytes: saliency must be 1, 2 or 3");
    }
}

}  // extern "C"
