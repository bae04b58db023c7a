// C ABI of libhydragen_hip.so (see include/hydragen_hip.h): argument validation, shapes-only launch planning, workspace carving.
// No allocation, no synchronisation, no device reads on the host.  One translation unit per kernel family (api_attn, api_layer,
// api_logits, api_generate, api_kv, api_comm); this one holds the error string they all write through fail() (api_core.h).
#include <cstdarg>

#include "api_core.h"

static thread_local char g_err[512] = "";

int hyd::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" {

int hyd_version(void) { return HYD_VERSION; }

const char* hyd_last_error_string(void) { return g_err; }

}  // extern "C"
