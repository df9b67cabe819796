// The C ABI (include/lgteun_hip.h) as the library sees it: the only thing the shared object exports (everything else: -fvisibility=hidden).
// csrc takes the public header through this file alone, so no include order can declare an entry point hidden, and a source that defines one
// includes it by name: with the prototype in sight a definition that does not match it is a compile error.
#pragma once
#pragma GCC visibility push(default)
#include "../../include/lgteun_hip.h"
#pragma GCC visibility pop
