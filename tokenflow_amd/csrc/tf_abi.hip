// ABI version, thread-local error string and launch-plan recorder of libtokenflow_hip.so.
#include <stdarg.h>
#include <string.h>

#include "tf_common.h"

static thread_local char g_err[512] = "";

void tf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

thread_local TfPlanRec* tf_plan_rec = nullptr;

bool tf_plan_note(const char* fmt, ...) {
    TfPlanRec* r = tf_plan_rec;
    if (!r) return false;
    char tok[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tok, sizeof(tok), fmt, ap);
    va_end(ap);
    const size_t need = strlen(tok) + (r->n ? 1 : 0);
    if (r->buf && r->used + need < r->len) snprintf(r->buf + r->used, r->len - r->used, "%s%s", r->n ? ";" : "", tok);
    r->used += need;
    ++r->n;
    return true;
}

extern "C" int tf_abi_version(void) { return TF_ABI_VERSION; }
extern "C" const char* tf_last_error(void) { return g_err; }
