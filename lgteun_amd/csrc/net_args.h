// The argument contract of the network entries (include/lgteun_hip.h, "The network entries' argument contract"): ONE validator that every one of
// them calls before its first HIP call (the workspace size among its checks).  Host code only; defined in api.hip.
#pragma once
#include <stdarg.h>
#include "common.h"

// Largest batch the network entries accept for a plan's (C, K, H, W) and `train` (as for lg_workspace_bytes); the header states the formula and
// tests/test_net_abi_cpu.py restates it.  The derivation, one line per limiting site, stands at the definition (api.hip).
int64_t lg_net_max_batch(const lg_config& c, int train);

// every flag bit the header defines, and the bits that belong to lgteun_backward alone
#define LG_FLAGS_DEFINED (LG_FLAG_FAITHFUL | LG_FLAG_SAVE | LG_FLAG_DROPOUT | LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA | LG_FLAG_CHAINED | LG_FLAG_DEFER_DEAD | \
                          LG_FLAG_STAGEWISE | LG_FLAG_LIVE_APART)
#define LG_FLAGS_FORWARD (LG_FLAGS_DEFINED & ~(LG_FLAG_BWD_LGT | LG_FLAG_BWD_DATA))

// One entry's checks, in the order the entry lists them.  The first failure writes "<who>: <argument> ..." to lg_last_error and sets rc; every later
// check is then a no-op, so an entry reads  `NetArgs v("op_lgt"); v.plan(p).f32(z, "z") ... ; if (v.rc) return v.rc;`
struct NetArgs {
    const char* who;
    int rc = 0;
    const lg_plan* pl = nullptr;
    explicit NetArgs(const char* w) : who(w) {}
    NetArgs& fail(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
    // -1: a null pointer, by name
    NetArgs& ptr(const void* p, const char* name) { return (rc || p) ? *this : fail(-1, "%s is NULL", name); }
    NetArgs& plan(const lg_plan* p) { pl = p; return ptr(p, "plan"); }
    // -1: alignment (a null pointer passes: optional arguments)
    NetArgs& aligned(const void* p, const char* name, unsigned a) { return (rc || !((uintptr_t)p & (a - 1))) ? *this : fail(-1, "%s must be %u-byte aligned", name, a); }
    // a float tensor: not null, 16-byte aligned (the network and loss kernels read and write float4; for the rest it is the contract's uniform rule)
    NetArgs& f32(const void* p, const char* name) { return ptr(p, name).aligned(p, name, 16); }
    // -1: an integer argument outside lo .. hi
    NetArgs& range(long long v, const char* name, long long lo, long long hi) { return (rc || (v >= lo && v <= hi)) ? *this : fail(-1, "%s must be in %lld .. %lld (got %lld)", name, lo, hi, v); }
    NetArgs& stage(int st) { return rc ? *this : range(st, "stage", 0, pl->cfg.K - 1); }
    // -1: 1 <= B <= lg_net_max_batch(plan, train)
    NetArgs& batch(int B, int train);
    // -1: a flag bit the header does not define; -2: a defined bit that does not apply to this entry (`allowed`: the bits that do)
    NetArgs& flags(int fl, int allowed);
    // -1: null / not 256-byte aligned; -3: smaller than lg_workspace_bytes(plan, B, train).  Behind batch(): B is in range here.
    NetArgs& workspace(const void* ws, size_t bytes, int B, int train);
};
