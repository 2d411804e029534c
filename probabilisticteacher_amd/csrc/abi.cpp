// abi.cpp -- error reporting, the per-device CU count + version of libptmi355.so.
#include <stdarg.h>

#include "common.h"

static thread_local char g_err[512] = "";

void ptmi_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// a launch asks per call (35 convolutions per step); a benign race at worst writes the same value twice
int ptmi_device_cus()
{
    static int cus_by_dev[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64 && cus_by_dev[dev] > 0) return cus_by_dev[dev];
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) cus = 256;
    if (dev >= 0 && dev < 64) cus_by_dev[dev] = cus;
    return cus;
}

extern "C" {
const char* ptmi_last_error(void) { return g_err; }
int ptmi_abi_version(void) { return 1; }
}
