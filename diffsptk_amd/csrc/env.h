// The one parser of the DSA_* route switches (the table of record: INTEGRATION.md, "Environment switches"; the same rule in
// Python: diffsptk_amd/_lib.py).  Host only.  Nothing here caches: a switch follows the environment at every call.
#pragma once
#include <stdlib.h>

namespace dsa {

// the variable's value, "" when it is unset
inline const char* env_text(const char* name)
{
    const char* v = getenv(name);
    return v ? v : "";
}

// An optional '-' and 1 to 9 decimal digits, nothing else; any other value (unset, empty, spaces, trailing text) gives dflt.
// An on/off switch is env_int(name, d) != 0; a three-state one has dflt -1, 0 never, 1 always.
inline int env_int(const char* name, int dflt)
{
    const char* v = env_text(name);
    const bool neg = *v == '-';
    int n = 0, digits = 0;
    for (v += neg; *v >= '0' && *v <= '9' && digits < 10; ++v, ++digits) n = digits < 9 ? n * 10 + (*v - '0') : n;
    return *v || digits < 1 || digits > 9 ? dflt : (neg ? -n : n);
}

}  // namespace dsa
